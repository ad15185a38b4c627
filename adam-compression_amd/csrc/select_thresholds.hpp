// Selection, K3: the sampled thresholds of every tensor — SampleKeys (the key source of
// radix_select.hpp's k_rs_passes), k_rs_reset_samples, k_rs_small_multi. The workgroup
// that produces a tensor's threshold also resets its state (sel_init_tensor). Relies on
// select_state.hpp.
#pragma once
#include "select_state.hpp"

namespace dgc {
// Sample keys of the tensors (or |vec| itself for a direct tensor, N == S).
struct SampleKeys {
    SelWS w;
    const float* vec_flat;
    __device__ __forceinline__ int task(int b) const { return task_of_block(w.bt[BT_SAMP], w.T, b); }
    __device__ __forceinline__ int first_block(int t) const { return w.bt[BT_SAMP][t]; }
    // participating workgroups: all of the task's for the samples; for the window list
    // (~3 ks keys) one per 4096 keys — 512 workgroups over 83k clustered keys paid
    // their histogram flushes on the same few bins and a 512-way arrival per pass
    __device__ __forceinline__ int blocks(int t) const {
        const int all = w.bt[BT_SAMP][t + 1] - w.bt[BT_SAMP][t];
        const uint32_t wn = w.rs[t].win_n;
        return wn ? min(all, (int)((wn + 4095u) / 4096u)) : all;
    }
    // a windowed task whose window k_rs_small_multi selected in one workgroup is done
    __device__ __forceinline__ bool active(int t) const {
        return !(w.td[t].win_cap > 0 && !w.td[t].tail && w.rs[t].small_done);
    }
    __device__ __forceinline__ RSState* state(int t) const { return w.rs + t; }
    __device__ __forceinline__ float* out(int t) const { return w.thr + t; }
    __device__ __forceinline__ uint32_t* chain() const { return w.chain + kChainOneWords; }   // k_rs_passes
    // the final pass's last workgroup: the threshold is known, reset the selection state
    __device__ __forceinline__ void done(int t) const { sel_init_tensor(w, t, 1); }
    template <class F>
    __device__ __forceinline__ void visit(int t, int64_t lb, int64_t nb, F&& f) const {
        const TDesc d = w.td[t];   // by value: stores below cannot alias it
        const uint32_t wn = w.rs[t].win_n;
        if (wn) {
            visit_dense(w.samples + d.win_off, wn, lb, nb, f);
            return;
        }
        const float* x = d.samp_off < 0 ? vec_flat + d.off : w.samples + d.samp_off;
        visit_dense(x, w.scnt[t], lb, nb, f);
    }
};

// Resets the radix state of every multi-block threshold task with its k (top_k_samples)
// and picks its keys. K1 appended every sample with key >= key(t_list) to the tensor's
// window list; when that list is complete (count <= win_cap) and holds >= ks keys,
// the ks-th largest sample is the ks-th largest of the list — every key above it is
// in the list, NaN and inf keys included — so the three passes read the list (~3 ks
// keys in the steady state) instead of the S samples. The result is the same either
// way. An unpadded tail's samples are written outside K1: no list then.
// ks1 > 0: tensor 0's top_k_samples (the one-tensor compress: dgc_compress_begin's
// table was laid out without it, and this saves re-uploading the table).
__device__ __forceinline__ int64_t ks_of(const TDesc& d, int t, int64_t ks1) { return ks1 > 0 && t == 0 ? ks1 : d.ks; }

__global__ void __launch_bounds__(kBlock) k_rs_reset_samples(SelWS w, int64_t ks1) {
    const int t = blockIdx.x;
    if (w.bt[BT_SAMP][t + 1] == w.bt[BT_SAMP][t]) return;
    const TDesc d = w.td[t];   // by value: stores below cannot alias it
    if (d.win_cap > 0 && !d.tail) return;   // windowed: k_rs_small_multi reset it (or selected its window)
    rs_reset(w.rs + t, (uint64_t)ks_of(d, t, ks1));
}

// One workgroup per small tensor: all three passes from LDS, then the tensor's
// selection state reset (sel_init_tensor). Workgroups nsmall.. take the windowed
// tensors (K1 appended every sample >= the list threshold to a window list): a
// complete window of ks..kSmallN keys is selected the same way, in ONE workgroup, and
// the multi-workgroup passes skip the tensor (small_done) — the ks-th largest sample is
// the ks-th largest of its window (SampleKeys); for VGG-16-BN's big tensors ~3 ks keys,
// where the passes were four launches. A window that does not qualify is left to them.
__global__ void __launch_bounds__(kScanThreads) k_rs_small_multi(SelWS w, const float* vec_flat, int64_t ks1,
                                                                 int32_t nsmall) {
    const int t = w.small[blockIdx.x];
    const TDesc d = w.td[t];   // by value: stores below cannot alias it
    const uint64_t ks = (uint64_t)ks_of(d, t, ks1);
    if ((int32_t)blockIdx.x >= nsmall) {
        const SelState* st = w.st + t;
        const uint32_t cnt = st->win_cnt[st->epoch & 1];
        const bool complete = cnt >= ks && cnt <= (uint64_t)d.win_cap;
        uint32_t* gh = reinterpret_cast<uint32_t*>(w.samples + d.whist_off);
        bool take = false;
        if (complete) {   // K1's histogram of the window first (it re-zeroes it), then its keys
            take = rs_window_hist_wg(w.samples + d.win_off, cnt, gh, st->win_key, (uint32_t)ks, w.thr + t);
            if (!take && cnt <= (uint32_t)kWinMax) {
                rs_window_wg(w.samples + d.win_off, cnt, ks, w.thr + t);
                take = true;
            }
        } else {
            for (int q = threadIdx.x; q < kWinBins; q += kScanThreads) gh[q] = 0;   // zero at rest
        }
        if (!take) {   // the multi-block passes take the task: its reset (their k, and the
            // window's keys instead of the samples when the window is complete)
            rs_reset(w.rs + t, ks);
            if (threadIdx.x == 0) {
                w.rs[t].small_done = 0u;
                w.rs[t].win_n = complete ? cnt : 0u;
            }
            return;
        }
        if (threadIdx.x == 0) {
            w.rs[t].small_done = 1u;
            w.rs[t].win_n = cnt;   // the record's window_keys (sel_init_tensor)
        }
        sel_init_tensor(w, t, 1);
        return;
    }
    const float* x = d.samp_off < 0 ? vec_flat + d.off : w.samples + d.samp_off;
    rs_small_wg(x, w.scnt[t], ks, w.thr + t);
    sel_init_tensor(w, t, 1);
    RS_STAMP(10);
}
}  // namespace dgc
