// Selection, K1: compensate + strided sample + the speculative candidate lists
// (k_compensate_list), and k_no_lists for a call whose vec no K1 listed. Relies on
// select_layout.hpp (OneTable, StartChunk) and select_tiles.hpp (loads, list_append,
// the deferred masking).
#pragma once
#include "select_tiles.hpp"

namespace dgc {
// K1 (compensate + strided sample, see compensate.hip) that also lists every
// element with |vec_new| >= t_list into its segment's list. One wave per segment:
// float4 index = 256*seg + 64*u + lane (u = 0..3), each instruction 1 KB contiguous;
// non-temporal loads and stores. seg_lcnt = exact count at t_list; a segment that
// holds an unpadded scalar tail is marked spilled (re-read when needed).
// ONE (a one-tensor call): the tensor's tables ride in the arguments (ot) — block 0
// writes them into the workspace for the kernels after K1, which replaces a k_put_one
// launch before every K1 (and its wait) — and the sample start in sc.
// CLIP: the gradient clipped as it is loaded (dgc_common.hpp clip1), tensor t's
// coefficient from ca; DGC_CLIP_NONE compiles to the unclipped kernel.
template <bool NEST, bool ONE, int CLIP>
__global__ void __launch_bounds__(kBlock)
k_compensate_list(const float* __restrict__ g_flat, float* __restrict__ mmt_flat, float* __restrict__ vec_flat,
                  float mom, SelWS w, StartChunk sc, int wt, OneTable ot, ClipArg ca) {
    const int t = ONE ? 0 : task(w, BT_K1, blockIdx.x);
    const TDesc d = ONE ? ot.d : w.td[t];   // by value: stores below cannot alias it
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b0 = ONE ? 0 : w.bt[BT_K1][t];   // the tensor's first block
    const int64_t ls = ((int64_t)blockIdx.x - b0) * kSegPerBlock4 + wave;   // local segment
    if (ONE && blockIdx.x == 0 && threadIdx.x == 0) {
        w.td[0] = ot.d;
        for (int which = 0; which < BT_COUNT; ++which) {
            w.bt[which][0] = ot.bt[which][0];
            w.bt[which][1] = ot.bt[which][1];
        }
        w.small[0] = 0;
    }
    // sample starts (and gradient pointers) of the first sc.count tensors ride in the arguments
    const bool arg_start = t < sc.count;
    const float* gsrc = !sc.ptrs ? g_flat + d.off : (arg_start ? sc.grad[t] : w.gptr[t]);
    const float4* g = reinterpret_cast<const float4*>(gsrc);
    float4* mmt = reinterpret_cast<float4*>(mmt_flat + d.off);
    float4* vec = reinterpret_cast<float4*>(vec_flat + d.off);
    const int64_t n4 = d.nv4, n = d.n;
    const float tl = w.spec ? w.spec[kSpecWords * t] : __builtin_huge_valf();
    SelState* st = w.st + t;
    if (blockIdx.x == b0 && threadIdx.x == 0) st->t_list = tl;
    const bool sample = d.samp_off >= 0;
    const int64_t start = !sample ? 0 : (arg_start ? sc.start[t] : w.starts[t]);
    const int64_t scount = !sample ? 0 : (arg_start ? ceil_div(d.n - start, d.stride) : w.scnt[t]);
    if (arg_start && blockIdx.x == b0 && threadIdx.x == 0) {
        w.starts[t] = sc.start[t];
        w.scnt[t] = sample ? scount : d.n;
    }
    float* sout = sample ? w.samples + d.samp_off : nullptr;
    // the sample window list: every sample with key >= the window threshold spec[2] (a
    // prediction of this call's sampled threshold, just below it; the list threshold
    // before the first prediction), inf and NaN too
    float* win = w.samples + d.win_off;
    const float tw = w.spec ? w.spec[kSpecWords * t + 2] : __builtin_huge_valf();
    const uint32_t win_key = abs_key(tw < __builtin_huge_valf() ? tw : tl);
    const bool windowed = sample && d.win_cap > 0;
    uint32_t* win_cnt = &st->win_cnt[st->epoch & 1];
    uint32_t* whist = reinterpret_cast<uint32_t*>(w.samples + d.whist_off);
    if (windowed && blockIdx.x == b0 && threadIdx.x == 0) st->win_key = win_key;
    // waves past the tensor's last segment load nothing and list nothing, but stay for
    // the block barrier of the spill count
    int64_t q0 = 0, r0 = 0;
    if (sample) floor_divmod_fast(ls * kSeg - start, d.stride, d.inv_stride, q0, r0);
    float4 gv[kSegTiles], mv[kSegTiles], vv[kSegTiles];
    const float cf = clip_coef<CLIP>(ca, t);
#pragma unroll
    for (int u = 0; u < kSegTiles; ++u) {
        const int64_t v = ls * (kSeg / 4) + u * 64 + lane;
        if (v < n4) {
            gv[u] = clip4<CLIP>(sc.ptrs && 4 * v + 3 >= n ? ld_tail4(gsrc, 4 * v, n) : ld_nt(g + v), cf);
            mv[u] = ld_nt(mmt + v);
            vv[u] = ld_nt(vec + v);
        }
    }
    uint32_t c = 0, mk = 0;
    const int64_t seg = d.seg0 + ls;
    uint16_t* lo = w.lst_off;
    float* lv = w.lst_val;
    if (st->def_mode && ls < d.nseg) apply_deferred_mask(*st, w, d, ls, lane, vv, mv);
#pragma unroll
    for (int u = 0; u < kSegTiles; ++u) {
        const int64_t v = ls * (kSeg / 4) + u * 64 + lane;
        const bool ok = v < n4;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        uint32_t valid = 0;
        bool hit = false;   // this lane's sample (at most one per float4: stride >= 4) joins the window
        float hv = 0.f;
        if (ok) {
            x[0] = comp1<NEST, true>(gv[u].x, mv[u].x, vv[u].x, mom);
            x[1] = comp1<NEST, true>(gv[u].y, mv[u].y, vv[u].y, mom);
            x[2] = comp1<NEST, true>(gv[u].z, mv[u].z, vv[u].z, mom);
            x[3] = comp1<NEST, true>(gv[u].w, mv[u].w, vv[u].w, mom);
            st_stream(mmt + v, mv[u], wt);
            st_stream(vec + v, vv[u], wt);
            const int64_t e = 4 * v;
            valid = e + 3 < n ? 0xFu : (e + 2 < n ? 7u : (e + 1 < n ? 3u : (e < n ? 1u : 0u)));
            if (sample) {
                const uint32_t tt = (uint32_t)r0 + 4u * (uint32_t)(u * 64 + lane);
                const uint32_t s32 = (uint32_t)d.stride;
                uint32_t q1, r;
                divmod_u32(tt, s32, d.inv_stride_f, q1, r);
                const uint32_t j = r == 0 ? 0u : s32 - r;
                if (j < 4 && ((valid >> j) & 1u)) {
                    const int64_t qi = q0 + q1 + (r == 0 ? 0 : 1);
                    if (qi >= 0 && qi < scount) {
                        hv = fabsf(x[j]);
                        sout[qi] = hv;
                        hit = windowed && __float_as_uint(hv) >= win_key;
                    }
                }
            }
        }
        const uint64_t hb = __ballot(hit);
        if (hb) {   // wave-uniform and rare (~3 ks of the S samples): one atomic per wave
            const int leader = __ffsll((unsigned long long)hb) - 1;
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(win_cnt, (uint32_t)__popcll(hb));
            base = __shfl(base, leader);
            const uint32_t pos = base + (uint32_t)__popcll(hb & ((1ull << lane) - 1));
            if (hit && pos < (uint64_t)d.win_cap) win[pos] = hv;
            if (hit) atomicAdd(&whist[win_bin(__float_as_uint(hv), win_key)], 1u);   // (no return value)
        }
        list_append(ge_mask(x, valid, tl), x, u * 256, c, lo, lv, seg);
        mk = max(mk, tile_max_key(x, valid));
    }
    const bool spilled = c > (uint32_t)kCap;
    mk = wave_max(mk);
    if (lane == 0 && ls < d.nseg) {
        const bool tail = d.tail && ls == d.nseg - 1;   // its scalar tail is compensated outside K1
        w.seg_lcnt[seg] = tail ? lcnt_pack(kCap + 1, 0xFFFFu) : lcnt_pack(c, lmax_code(mk));
    }
    // one atomic per workgroup with a spilled segment (shard by block)
    const uint64_t any = __ballot(spilled);
    __shared__ uint32_t nsp;
    if (threadIdx.x == 0) nsp = 0;
    __syncthreads();
    if (lane == 0 && any) atomicAdd(&nsp, 1u);
    __syncthreads();
    if (threadIdx.x == 0 && nsp) atomicAdd(&st->spill[st->epoch & 1][blockIdx.x % kSpillShards], nsp);
}

__global__ void k_no_lists(SelWS w) {
    for (int t = threadIdx.x; t < w.T; t += blockDim.x) w.st[t].t_list = __builtin_huge_valf();
}
}  // namespace dgc
