// Selection, K1 for fp32 state under a 16-bit gradient (bf16 / fp16): k_compensate_list_g16,
// the flat bucket's one-tensor, unclipped K1 with the gradient widened in its load, and
// k_compensate_tail_g16, the scalar tail of an unpadded tensor. The reference's
// DGCSGDMemory.compensate on fp32 momentum / velocity and a 16-bit gradient
// (dgc/memory.py:50-63) runs every op in fp32 on the exactly widened gradient (torch's type
// promotion of the in-place ops), so the step is bit for bit the fp32 one on grad.float():
// everything here but the gradient's stream is k_compensate_list<NEST, true, DGC_CLIP_NONE>.
// A sibling kernel, not one more template parameter of k_compensate_list: that would rename
// its instantiations and could change their code (tools/kernel_hashes.py).
//
// Layout: the fp32 kernel's. One wave per segment, element group (4 elements) index =
// 256*seg + 64*u + lane (u = 0..3): a 16-B load per lane of momentum and velocity (1 KB
// contiguous per instruction), an 8-B load per lane of the gradient (512 B per instruction,
// K1-16's ld_nt / unpack4), so the lane-to-element mapping, list_append, the sample
// arithmetic and the list order are the fp32 kernel's. 18 B/elem where grad.float() and the
// fp32 kernel move 6 + 20.
//
// Schedule: as select_k1.hpp documents. The state words are independent loads of wave-uniform
// addresses ahead of any store, and the wave's twelve streaming loads (eight 16-B, four 8-B)
// go out through global-typed pointers before the first use of either kind: 10 KB in flight
// per wave. The launch keeps the fp32 flat launch's policy (select.hip, kK1FlatLds).
//
// Bounds: the state is unpadded (d.nv4 = n / 4 full groups), and the gradient is exactly n
// elements: a live lane loads group gi of all three arrays only while gi < n / 4, so the
// last byte read is below element 4 * (n / 4) <= n of each. The n & 3 elements after it are
// compensated by k_compensate_tail_g16 from 2-B loads of the gradient; their samples are
// read back from vec and their segment is marked spilled (d.tail), as dgc_compress_begin
// does.
#pragma once
#include "select_k1_16.hpp"

namespace dgc {
template <int GD, bool NEST>
__global__ void __launch_bounds__(kBlock)
k_compensate_list_g16(const uint16_t* __restrict__ g16, float* __restrict__ mmt_flat, float* __restrict__ vec_flat,
                      float mom, SelWS w, int64_t start, int wt, OneTable ot) {
    const TDesc d = ot.d;   // by value: stores below cannot alias it
    const int lane = threadIdx.x & 63, wave = wave_id();
    const int64_t ls = (int64_t)blockIdx.x * kSegPerBlock4 + wave;   // local segment
    // a wave past the last segment loads nothing and lists nothing (no early exit: a
    // branch here would split the state reads from the streaming loads)
    const bool live = ls < d.nseg;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    const bool sample = d.samp_off >= 0;

    // ---- the state words, one batch (uses further down)
    DGC_GLB SelState* st = glb(w.st);
    DGC_GLB const float* spec = w.spec ? glb(w.spec) : &st->t0;   // (null: any readable words)
    const float spec0 = spec[0], spec2 = spec[2];
    const int32_t epoch = st->epoch, def_mode = st->def_mode, def_mask_mmt = st->def_mask_mmt;
    const float def_t = st->def_t;
    const long long def_limit = st->def_limit;
    // the deferred masking's offsets: the slots exist for ls < d.nseg whether or not a
    // masking is pending, and their addresses come from the arguments
    const int64_t lsd = live ? ls : 0;
    DGC_GLB const long long* grp_off = glb(w.grp_off) + (d.grp0 + lsd / kGroupSegs);
    DGC_GLB const uint32_t* seg_off = glb(w.seg_off) + (d.seg0 + lsd);
    const long long def_rank = *grp_off + (long long)*seg_off;

    // ---- the streaming loads: momentum and velocity, then the gradient's full groups
    const int64_t n = d.n;
    const int64_t seg4 = ls * (kSeg / 4);
    const int left = (int)min(d.nv4 - seg4, (int64_t)(kSeg / 4));   // full groups of the segment
    DGC_GLB float4* mmt = glb(reinterpret_cast<float4*>(mmt_flat + d.off) + seg4);
    DGC_GLB float4* vec = glb(reinterpret_cast<float4*>(vec_flat + d.off) + seg4);
    DGC_GLB const u2v* g = glb(reinterpret_cast<const u2v*>(g16 + d.off) + seg4);
    float4 mv[kSegTiles], vv[kSegTiles];
    uint2 gv[kSegTiles];
#pragma unroll
    for (int u = 0; u < kSegTiles; ++u) {
        if (u * 64 + lane < left) {
            mv[u] = ld_nt(mmt + u * 64 + lane);
            vv[u] = ld_nt(vec + u * 64 + lane);
        }
    }
#pragma unroll
    for (int u = 0; u < kSegTiles; ++u)
        if (u * 64 + lane < left) gv[u] = ld_nt(g + u * 64 + lane);

    // ---- everything loaded is in flight: the stores of the call's tables
    if (first) {
        w.td[0] = ot.d;
        for (int which = 0; which < BT_COUNT; ++which) {
            w.bt[which][0] = ot.bt[which][0];
            w.bt[which][1] = ot.bt[which][1];
        }
        w.small[0] = 0;
    }
    if (!sample) start = 0;
    const int64_t scount = !sample ? 0 : ceil_div(d.n - start, d.stride);
    const K1Seg k = k1_segment_begin(w, d, 0, st, first, true, spec0, spec2, epoch, ls, start, scount);
    uint32_t c = 0, mk = 0;
    const int64_t seg = d.seg0 + ls;
    if (def_mode && live) apply_deferred_mask(def_t, def_limit, def_mask_mmt != 0, def_rank, d, ls, lane, vv, mv);
#pragma unroll
    for (int u = 0; u < kSegTiles; ++u) {
        const bool ok = u * 64 + lane < left;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        uint32_t valid = 0;
        bool hit = false;   // this lane's sample (at most one per group: stride >= 4) joins the window
        float hv = 0.f;
        if (ok) {
            float gx[4];
            unpack4<GD>(gv[u], gx);   // exact: the reference's promotion of the 16-bit gradient
            x[0] = comp1<NEST, true>(gx[0], mv[u].x, vv[u].x, mom);
            x[1] = comp1<NEST, true>(gx[1], mv[u].y, vv[u].y, mom);
            x[2] = comp1<NEST, true>(gx[2], mv[u].z, vv[u].z, mom);
            x[3] = comp1<NEST, true>(gx[3], mv[u].w, vv[u].w, mom);
            st_stream(mmt + u * 64 + lane, mv[u], wt);
            st_stream(vec + u * 64 + lane, vv[u], wt);
            const int64_t e = 4 * (seg4 + u * 64 + lane);
            valid = e + 3 < n ? 0xFu : (e + 2 < n ? 7u : (e + 1 < n ? 3u : (e < n ? 1u : 0u)));
            if (sample) hit = k1_sample(k, d, x, valid, u * 64 + lane, k.windowed, hv);
        }
        k1_window_append(k, d.win_cap, hit, hv, lane);
        list_append(ge_mask(x, valid, k.tl), x, u * 256, c, w.lst_off, w.lst_val, seg);
        mk = max(mk, tile_max_key(x, valid));
    }
    // (the segment with the scalar tail, compensated by k_compensate_tail_g16, is marked spilled)
    k1_segment_end(c, mk, lane == 0 && live, d.tail && ls == d.nseg - 1, w.seg_lcnt + seg, w.st[0].spill[epoch & 1]);
}

// The n & 3 elements [begin, n) after the last full group: comp1 on the widened gradient,
// one thread each (k_compensate1's arithmetic, compensate.hip, with the 16-bit read).
template <int GD, bool NEST>
__global__ void k_compensate_tail_g16(const uint16_t* __restrict__ g16, float* __restrict__ mmt, float* __restrict__ vec,
                                      int64_t begin, int64_t n, float mom) {
    const int64_t i = begin + threadIdx.x;
    if (i >= n) return;
    float mv = mmt[i], vv = vec[i];
    comp1<NEST, true>(h16_to_f32<GD>(g16[i]), mv, vv, mom);
    mmt[i] = mv;
    vec[i] = vv;
}
}  // namespace dgc
