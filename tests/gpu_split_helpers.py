"""What the split-exchange tests share (test_gpu_split.py, test_gpu_k6_edges.py): a rank's packed
payload on the device and ``Split`` — W ranks' payloads split by dgc_payload_split, assembled
part-major as the ``parts`` allgathers would leave them, and scattered phase by phase."""
import ctypes

import numpy as np
import torch

DEV = torch.device("cuda:0")


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def check(L, rc):
    assert rc == 0, L.dgc_last_error().decode()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rank_payload(L, v, i, cap, vd, idt):
    vo, io = ctypes.c_int64(0), ctypes.c_int64(0)
    stride = L.dgc_payload_layout(cap, vd, idt, ctypes.byref(vo), ctypes.byref(io))
    p = np.zeros(stride, np.uint8)
    v = v.astype(np.float16 if vd else np.float32)
    i = i.astype(np.int32 if idt else np.int64)
    p[:8] = np.frombuffer(np.int64(len(i)).tobytes(), np.uint8)
    p[vo.value: vo.value + v.nbytes] = np.frombuffer(v.tobytes(), np.uint8)
    p[io.value: io.value + i.nbytes] = np.frombuffer(i.tobytes(), np.uint8)
    return torch.from_numpy(p).to(DEV)


class Split:
    def __init__(self, L, N, W, parts, cap, vd, idt):
        self.L, self.N, self.W, self.parts, self.cap, self.vd, self.idt = L, N, W, parts, cap, vd, idt
        pc = ctypes.c_int64(0)
        self.pbytes = L.dgc_payload_split_layout(cap, parts, vd, idt, ctypes.byref(pc))
        self.pc = pc.value
        self.sbytes = L.dgc_payload_split_bytes(cap, parts, vd, idt)
        assert self.sbytes >= parts * self.pbytes
        self.split = torch.zeros(self.sbytes, dtype=torch.uint8, device=DEV)   # scratch zero at rest
        wsz = L.dgc_decompress_split_workspace(N, W, parts, cap)
        assert wsz > 0
        self.ws = torch.empty(wsz, dtype=torch.uint8, device=DEV)

    def gather(self, runs):
        """Every rank's payload split on the device and placed part-major (the collectives' output)."""
        L, pb, W = self.L, self.pbytes, self.W
        g = torch.zeros(self.parts * W * pb, dtype=torch.uint8, device=DEV)
        heads = []
        for r, (v, i) in enumerate(runs):
            pay = _rank_payload(L, v, i, self.cap, self.vd, self.idt)
            check(L, L.dgc_payload_split(P(pay), self.cap, self.parts, self.vd, self.idt, P(self.split), stream()))
            for p in range(self.parts):
                g[(p * W + r) * pb: (p * W + r + 1) * pb].copy_(self.split[p * pb: (p + 1) * pb])
            heads.append(self.split[: self.parts * pb].view(self.parts, pb)[:, :16].clone().view(torch.int64))
        assert int(self.split[self.parts * pb:].count_nonzero()) == 0   # scratch left zero
        return g, heads

    def scatter(self, g, out, cleared, want=None):
        for p in range(self.parts):
            check(self.L, self.L.dgc_scatter_split(P(g), self.W, self.parts, p, self.cap, self.vd, self.idt, P(out),
                                                   self.N, 1.0 / self.W, int(cleared and p == 0), P(self.ws),
                                                   self.ws.numel(), stream()))
            if want is not None and p < self.parts - 1:   # every value written so far is final
                o = out.cpu().numpy()
                nz = o != 0
                assert np.array_equal(bits(o[nz]), bits(want[nz])), p

    def status(self):
        st = ctypes.c_int32(-1)
        check(self.L, self.L.dgc_decompress_status(P(self.ws), ctypes.byref(st), stream()))
        return st.value
