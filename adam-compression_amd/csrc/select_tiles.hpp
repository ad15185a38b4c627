// Selection, tile helpers: the float4 tile loads (ld_tail4, load_tile), the list count
// packing (lmax_code, lcnt_*), ge_mask and list_append for the listing stages (K1, the
// select pass), task() — a workgroup's tensor from a block table, used by every stage —
// and the deferred momentum masking (k_mask_flush, k_def_clear, mask_flush). Relies on
// select_types.hpp and, for mask_flush's grid, select_layout.hpp.
#pragma once
#include "select_layout.hpp"

namespace dgc {
// The last float4 of a pointer-table gradient that ends inside it (exactly n floats long,
// n & 3 of them in this float4, which starts at element 4 * (n / 4)): elements past n
// read as 0. Scalar loads: a 16-B load would run past the gradient's end.
__device__ __forceinline__ float4 ld_tail4(DGC_GLB const float* g, int64_t n) {
    DGC_GLB const float* p = g + (n & ~(int64_t)3);
    const int r = (int)(n & 3);
    return make_float4(p[0], r > 1 ? p[1] : 0.f, r > 2 ? p[2] : 0.f, 0.f);
}

// Upper bound of a segment's largest |x| key, in 16-bit units: every key < code << 16.
// k_count_lists skips the list of a segment whose code says every |x| < t_cur — at
// 7B most lists hold an entry or two below t_cur, and reading them cost a 128-B line
// per segment. NaN keys give codes above any finite threshold's key (never skipped).
__device__ __forceinline__ uint32_t lmax_code(uint32_t max_key) { return (max_key >> 16) + 1; }
// seg_lcnt packs the list count (<= kSeg) with the code: one 4-B store per segment
__device__ __forceinline__ uint32_t lcnt_pack(uint32_t count, uint32_t code) { return count | (code << 16); }
__device__ __forceinline__ uint32_t lcnt_count(uint32_t v) { return v & 0xFFFFu; }
__device__ __forceinline__ uint32_t tile_max_key(const float (&x)[4], uint32_t valid) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if ((valid >> j) & 1u) m = max(m, abs_key(x[j]));
    return m;
}

// Lane holds elements e0..e0+3 of a 256-element tile (e0 = tile base + 4*lane) of a
// tensor whose elements start at v (local indices, n of them).
template <bool ALIGNED>
__device__ __forceinline__ void load_tile(const float* __restrict__ v, int64_t n, int64_t e0, float (&x)[4],
                                          uint32_t& valid) {
    if (ALIGNED && e0 + 3 < n) {
        const float4 q = ld_nt(reinterpret_cast<const float4*>(v + e0));
        x[0] = q.x;
        x[1] = q.y;
        x[2] = q.z;
        x[3] = q.w;
        valid = 0xFu;
    } else {
        valid = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = e0 + j < n;
            x[j] = ok ? v[e0 + j] : 0.f;
            valid |= (uint32_t)ok << j;
        }
    }
}

__device__ __forceinline__ uint32_t ge_mask(const float (&x)[4], uint32_t valid, float t) {
    uint32_t p = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) p |= (uint32_t)(fabsf(x[j]) >= t) << j;
    return p & valid;
}

// Append the lanes' flagged elements (element order 4*lane + j) to a segment list
// (lo / lv: its column, entries kLstTile apart).
__device__ __forceinline__ void list_append(uint32_t p, const float (&x)[4], int tile_off, uint32_t& c,
                                            uint16_t* lo, float* lv, int64_t seg) {
    if (__ballot(p != 0)) {
        uint32_t lb, tot;
        wave_prefix4(p, lb, tot);
        uint32_t r = c + lb;
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (p & (1u << j)) {
                if (r < (uint32_t)kCap) {
                    lo[lslot(seg, r)] = (uint16_t)(tile_off + 4 * lane + j);
                    lv[lslot(seg, r)] = x[j];
                }
                ++r;
            }
        }
        c += tot;
    }
}

// The calling wave's view of local segment ls of a tensor (elements v[0..n)):
// tile u holds elements ls*1024 + 256u + 4*lane + j. All loads are issued before
// any use; 16-B loads when the tensor base is 16-B aligned (a uniform branch).
__device__ __forceinline__ void load_segment(const float* __restrict__ v, int64_t n, int64_t ls,
                                             float (&x)[kSegTiles][4], uint32_t (&valid)[kSegTiles]) {
    const int lane = threadIdx.x & 63;
    if (aligned16(v)) {
#pragma unroll
        for (int u = 0; u < kSegTiles; ++u) load_tile<true>(v, n, ls * kSeg + u * 256 + 4 * lane, x[u], valid[u]);
    } else {
#pragma unroll
        for (int u = 0; u < kSegTiles; ++u) load_tile<false>(v, n, ls * kSeg + u * 256 + 4 * lane, x[u], valid[u]);
    }
}

// Count of |x| >= t over local segment ls of a tensor, re-read by the calling wave.
__device__ uint32_t wave_count_segment(const float* __restrict__ v, int64_t n, int64_t ls, float t) {
    float x[kSegTiles][4];
    uint32_t valid[kSegTiles];
    load_segment(v, n, ls, x, valid);
    uint32_t c = 0;
#pragma unroll
    for (int u = 0; u < kSegTiles; ++u) c += __popc(ge_mask(x[u], valid[u], t));
    return wave_sum(c);
}

__device__ __forceinline__ int task(const SelWS& w, int which, int b) { return task_of_block(w.bt[which], w.T, b); }

// The last call's deferred masking for one segment (one wave): zero, in the loaded
// tiles, the elements that call emitted — the first dlim elements (flat order) with
// |vec| >= dt, ranked from `rank` (the segment's grp_off + seg_off) by in-segment rank.
// vec is unchanged since that emit, so the recount reproduces its choice exactly. The
// caller passes the state words by value: K1 loads them ahead of its streaming loads.
__device__ __forceinline__ void apply_deferred_mask(float dt, long long dlim, bool mm, long long rank,
                                                    const TDesc& d, int64_t ls, int lane, float4 (&vv)[kSegTiles],
                                                    float4 (&mv)[kSegTiles]) {
#pragma unroll
    for (int u = 0; u < kSegTiles; ++u) {
        if (rank >= dlim) break;   // wave-uniform
        const int64_t v = ls * (kSeg / 4) + u * 64 + lane;
        const float xo[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
        const uint32_t pm = ge_mask(xo, v < d.nv4 ? 0xFu : 0u, dt);
        uint32_t lb, tot;
        wave_prefix4(pm, lb, tot);
        long long r = rank + lb;
        float* vf = reinterpret_cast<float*>(&vv[u]);
        float* mf = reinterpret_cast<float*>(&mv[u]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (pm & (1u << j)) {
                if (r < dlim) {
                    vf[j] = 0.f;
                    if (mm) mf[j] = 0.f;
                }
                ++r;
            }
        rank += tot;
    }
}

// Applies a pending deferred masking without compensating (flush before anyone reads
// vec/mmt, and the non-list K1 fallback). One wave per segment.
__global__ void __launch_bounds__(kBlock) k_mask_flush(float* __restrict__ vec_flat, float* __restrict__ mmt_flat,
                                                       SelWS w) {
    const int t = task(w, BT_K1, blockIdx.x);
    const SelState* st = w.st + t;
    if (!st->def_mode) return;
    const TDesc d = w.td[t];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ls = ((int64_t)blockIdx.x - w.bt[BT_K1][t]) * kSegPerBlock4 + wave;
    if (ls >= d.nseg) return;
    float* vec = vec_flat + d.off;
    float* mmt = st->def_mask_mmt ? mmt_flat + d.off : nullptr;
    const float dt = st->def_t;
    const long long dlim = st->def_limit;
    long long rank = w.grp_off[d.grp0 + ls / kGroupSegs] + w.seg_off[d.seg0 + ls];
    if (rank >= dlim) return;
    float x[kSegTiles][4];
    uint32_t valid[kSegTiles];
    load_segment(vec, d.n, ls, x, valid);
#pragma unroll
    for (int u = 0; u < kSegTiles; ++u) {
        const uint32_t pm = ge_mask(x[u], valid[u], dt);
        uint32_t lb, tot;
        wave_prefix4(pm, lb, tot);
        long long r = rank + lb;
        const int64_t e0 = ls * kSeg + u * 256 + 4 * lane;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (pm & (1u << j)) {
                if (r < dlim) {
                    vec[e0 + j] = 0.f;
                    if (mmt) mmt[e0 + j] = 0.f;
                }
                ++r;
            }
        rank += tot;
    }
}

__global__ void k_def_clear(SelWS w) {
    for (int t = threadIdx.x; t < w.T; t += blockDim.x) w.st[t].def_mode = 0;
}

static int mask_flush(float* vec, float* mmt, const Layout& L, const SelWS& w, hipStream_t s) {
    if (L.grid[BT_K1] > 0x7FFFFFFFLL) DGC_FAIL(DGC_ERR_INVALID, "dgc_compress: n too large");
    if (L.grid[BT_K1] > 0) {
        hipLaunchKernelGGL(k_mask_flush, dim3((unsigned)L.grid[BT_K1]), dim3(kBlock), 0, s, vec, mmt, w);
        DGC_LAUNCHED();
    }
    hipLaunchKernelGGL(k_def_clear, dim3(1), dim3(256), 0, s, w);
    DGC_LAUNCHED();
    return DGC_OK;
}
}  // namespace dgc
