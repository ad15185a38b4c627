// Selection, count passes: the profiling stamps (PASS_STAMP, ES_STAMP), the list count
// (count_lists_body, k_count_lists), the full select pass, their merged launch
// (k_count_pass) and the multi-threshold lowering (lower_counts_body, lower_lists_body).
// The *_body functions also serve select_emit.hpp (k_chain_one, k_count_emit). Relies on
// select_tiles.hpp (loads, list_append, task) and select_state.hpp (decide_tensor).
#pragma once
#include "select_tiles.hpp"
#include "select_state.hpp"

namespace dgc {
#ifdef DGC_K5_PROF
// tools/pass_prof.py: per-workgroup stamps of the last k_count_pass (kind 0) and
// k_lower_counts (kind 1) launch — entry, past the gate, loads done, arrival, end
__device__ unsigned long long g_pass_prof[2][16384][6];
#define PASS_STAMP(k, i) \
    do { if (threadIdx.x == 0 && blockIdx.x < 16384) g_pass_prof[k][blockIdx.x][i] = wall_clock64(); } while (0)
// slot 5: the first iteration's loads arrived (wave 0; the wait is the profiling build's only)
#define PASS_LOADED(k) \
    do { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); PASS_STAMP(k, 5); } while (0)
// tools/es_prof.py: k_emit_wide_t's workgroups — [0] entry, [1] emit: scan done / set:
// its tensor's gather complete, [2] done
__device__ unsigned long long g_es_prof[4096][3];
#define ES_STAMP(i) \
    do { if (threadIdx.x == 0 && blockIdx.x < 4096) g_es_prof[blockIdx.x][i] = wall_clock64(); } while (0)
#else
#define PASS_STAMP(k, i) do { } while (0)
#define PASS_LOADED(k) do { } while (0)
#define ES_STAMP(i) do { } while (0)
#endif
// t_cur >= t_list: counts from the lists, kCountSegs segments per thread (one group
// per workgroup): the list counts of a thread's segments, then their first 8 entries
// (most lists are shorter), are all in flight before any is used — one thread per
// segment paid two dependent round trips per segment in ~13 waves of workgroups at 7B.
// Spilled segments are re-read by the block's waves. One atomic per block into its group;
// the tensor's last workgroup then takes the adaptation step (decide_tensor).
static_assert(kBlock * kCountSegs == kGroupSegs, "k_count_lists: one group per workgroup");
__device__ __forceinline__ void count_lists_body(const float* __restrict__ vec_flat, const SelWS& w, const SelCfg& p,
                                                 int64_t bx) {
    const int t = task(w, BT_CNT, (int)bx);
    const SelState* st = w.st + t;
    PASS_STAMP(0, 0);
    if (!st->active || !(st->t_cur >= st->t_list)) return;
    PASS_STAMP(0, 1);
    const TDesc d = w.td[t];   // by value: stores below cannot alias it
    const float* vec = vec_flat + d.off;
    const float tc = st->t_cur;
    __shared__ int spill[kBlock * kCountSegs];
    __shared__ int nspill;
    __shared__ uint32_t bsum;
    if (threadIdx.x == 0) {
        nspill = 0;
        bsum = 0;
    }
    __syncthreads();
    const int64_t lseg0 = (bx - w.bt[BT_CNT][t]) * kBlock * kCountSegs;
    uint32_t lc[kCountSegs];
    const uint32_t tkey = abs_key(tc);
#pragma unroll
    for (int j = 0; j < kCountSegs; ++j) {
        const int64_t ls = lseg0 + j * kBlock + threadIdx.x;
        const uint32_t v = ls < d.nseg ? w.seg_lcnt[d.seg0 + ls] : 0u;
        // a segment whose every |x| is below t_cur counts 0 without reading its list
        // (or, spilled, its elements)
        lc[j] = ((v >> 16) << 16) <= tkey ? 0u : lcnt_count(v);
    }
    constexpr int kFirst = 8;   // entries loaded up front (one interleaved line)
    float a[kCountSegs][kFirst];
#pragma unroll
    for (int j = 0; j < kCountSegs; ++j) {
        const int64_t sj = d.seg0 + lseg0 + j * kBlock + threadIdx.x;
#pragma unroll
        for (int e = 0; e < kFirst; ++e)
            if ((uint32_t)e < lc[j] && lc[j] <= (uint32_t)kCap) a[j][e] = w.lst_val[lslot(sj, e)];
    }
    uint32_t ctot = 0;
#pragma unroll
    for (int j = 0; j < kCountSegs; ++j) {
        const int64_t ls = lseg0 + j * kBlock + threadIdx.x;
        if (ls >= d.nseg) continue;
        const int64_t seg = d.seg0 + ls;
        const uint32_t n = lc[j];
        if (n > (uint32_t)kCap) {
            spill[atomicAdd(&nspill, 1)] = j * kBlock + threadIdx.x;
            continue;
        }
        uint32_t c = 0;
#pragma unroll
        for (int e = 0; e < kFirst; ++e) c += (uint32_t)e < n && fabsf(a[j][e]) >= tc;
        // the rest of a longer list, 16 loads in flight at a time
        for (uint32_t e0 = kFirst; e0 < n; e0 += 16) {
            float v[16];
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (e0 + q < n) v[q] = w.lst_val[lslot(seg, e0 + q)];
#pragma unroll
            for (int q = 0; q < 16; ++q) c += e0 + q < n && fabsf(v[q]) >= tc;
        }
        w.seg_cnt[seg] = c;
        ctot += c;
    }
    ctot = wave_sum(ctot);
    if ((threadIdx.x & 63) == 0 && ctot) atomicAdd(&bsum, ctot);
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    for (int q = wave; q < nspill; q += kSegPerBlock4) {
        const int64_t ls2 = lseg0 + spill[q];
        const uint32_t cs = wave_count_segment(vec, d.n, ls2, tc);
        if ((threadIdx.x & 63) == 0) {
            w.seg_cnt[d.seg0 + ls2] = cs;
            if (cs) atomicAdd(&bsum, cs);
        }
    }
    __syncthreads();
    PASS_STAMP(0, 2);
    if (threadIdx.x == 0 && bsum) atomicAdd(&w.grp_cnt[d.grp0 + lseg0 / kGroupSegs], (unsigned long long)bsum);
    PASS_STAMP(0, 3);
    // the tensor's last workgroup takes the adaptation step (no k_decide launch)
    if (last_block_arrival8(w.st[t].tk8, (uint32_t)(bx - w.bt[BT_CNT][t]),
                            (uint32_t)(w.bt[BT_CNT][t + 1] - w.bt[BT_CNT][t])))
        decide_tensor(w, p, t);
    PASS_STAMP(0, 4);
}

__global__ void __launch_bounds__(kBlock)
k_count_lists(const float* __restrict__ vec_flat, SelWS w, SelCfg p) {
    count_lists_body(vec_flat, w, p, blockIdx.x);
}

// t_cur < t_list: full select pass at t_cur — one wave per SUPER segments (kSuper: 16
// float4 loads in flight per lane), re-lists every segment; seg_lcnt = seg_cnt.
// `which` = BT_FULL (one-shot) or BT_CAP16 (grid-stride within the tensor, for a
// launch that is most likely a gated no-op) — BT_K1 / BT_CAP4 for SUPER = 1. The
// tensor's last workgroup then takes the adaptation step (decide_tensor).
template <bool ALIGNED, int SUPER = kSuper>
__device__ __forceinline__ void select_pass_body(const float* __restrict__ vec_flat, const SelWS& w, int which,
                                                 const SelCfg& p, int64_t bx) {
    static_assert(kGroupSegs % (kSegPerBlock4 * SUPER) == 0, "a workgroup's segments lie in one group");
    const int t = task(w, which, (int)bx);
    const SelState* st = w.st + t;
    PASS_STAMP(0, 0);
    if (!st->active || st->t_cur >= st->t_list) return;
    PASS_STAMP(0, 1);
    const TDesc d = w.td[t];   // by value: stores below cannot alias it
    const float* vec = vec_flat + d.off;
    const float tc = st->t_cur;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int kTiles = SUPER * kSegTiles;   // 16 for kSuper
    __shared__ uint32_t wcnt[kSegPerBlock4];
    __shared__ uint32_t wovf[kSegPerBlock4];
    const int64_t nsuper = ceil_div(d.nseg, (int64_t)SUPER);
    const int64_t nb = w.bt[which][t + 1] - w.bt[which][t];
    for (int64_t bi = bx - w.bt[which][t]; bi * kSegPerBlock4 < nsuper; bi += nb) {
        const int64_t sup = bi * kSegPerBlock4 + wave;
        uint32_t ctot = 0, novf = 0;
        if (sup < nsuper) {
            float x[kTiles][4];
            uint32_t valid[kTiles];
#pragma unroll
            for (int u = 0; u < kTiles; ++u)
                load_tile<ALIGNED>(vec, d.n, sup * (SUPER * kSeg) + u * 256 + 4 * lane, x[u], valid[u]);
            PASS_LOADED(0);
#pragma unroll
            for (int sg = 0; sg < SUPER; ++sg) {
                const int64_t ls = sup * SUPER + sg;
                const int64_t seg = d.seg0 + ls;
                uint32_t c = 0;
                uint16_t* lo = w.lst_off;
                float* lv = w.lst_val;
                if (ls < d.nseg) {   // uniform per wave
                    uint32_t mk = 0;
#pragma unroll
                    for (int u = 0; u < kSegTiles; ++u) {
                        list_append(ge_mask(x[sg * kSegTiles + u], valid[sg * kSegTiles + u], tc),
                                    x[sg * kSegTiles + u], u * 256, c, lo, lv, seg);
                        mk = max(mk, tile_max_key(x[sg * kSegTiles + u], valid[sg * kSegTiles + u]));
                    }
                    mk = wave_max(mk);
                    if (lane == 0) {
                        w.seg_lcnt[seg] = lcnt_pack(c, lmax_code(mk));
                        w.seg_cnt[seg] = c;
                    }
                }
                ctot += c;
                novf += c > (uint32_t)kCap;
            }
        }
        if (lane == 0) {
            wcnt[wave] = ctot;
            wovf[wave] = novf;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t s = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
            const uint32_t o = wovf[0] + wovf[1] + wovf[2] + wovf[3];
            if (s) atomicAdd(&w.grp_cnt[d.grp0 + (bi * kSegPerBlock4 * SUPER) / kGroupSegs], (unsigned long long)s);
            if (o) atomicAdd(&w.st[t].overflow, (int)o);
        }
        __syncthreads();
    }
    PASS_STAMP(0, 2);
    PASS_STAMP(0, 3);
    // the tensor's last workgroup takes the adaptation step (no k_decide launch)
    if (last_block_arrival8(w.st[t].tk8, (uint32_t)(bx - w.bt[which][t]), (uint32_t)nb))
        decide_tensor(w, p, t);
    PASS_STAMP(0, 4);
}

template <bool ALIGNED>
__global__ void __launch_bounds__(kBlock)
k_select_pass(const float* __restrict__ vec_flat, SelWS w, int which, SelCfg p) {
    select_pass_body<ALIGNED>(vec_flat, w, which, p, blockIdx.x);
}

// One count pass as ONE launch: the list counts (the first ncnt workgroups) beside the
// full select pass (the rest) — a tensor takes one of the two (t_cur >= t_list or not),
// so the two run side by side instead of one launch after the other. Only for calls
// whose decide steps cannot leave a tensor active for a recount within the launch (the
// multi-threshold lowering: resample on, max_iters <= kMaxLower — then a decide either
// finishes the tensor or hands it to the lowering), so both gates read one state.
template <bool ALIGNED, int SUPER>
__global__ void __launch_bounds__(kBlock)
k_count_pass(const float* __restrict__ vec_flat, SelWS w, int which, SelCfg p, int ncnt) {
    if ((int)blockIdx.x < ncnt)
        count_lists_body(vec_flat, w, p, blockIdx.x);
    else
        select_pass_body<ALIGNED, SUPER>(vec_flat, w, which, p, (int64_t)blockIdx.x - ncnt);
}

// Counts at t_j = fl32(t_{j-1} * lower), j = 1..max_iters, in ONE pass over vec (the
// reference's "lower" recounts, dgc/compression.py:140-148, all at once). The last
// workgroup of the tensor picks j* = the first j whose count reaches lower*k (else
// max_iters) and arms the count pass + decide at t_{j*}.
template <bool ALIGNED, int SEGS = 1>
__device__ __forceinline__ void lower_counts_body(const float* __restrict__ vec_flat, const SelWS& w,
                                                  const SelCfg& p, int64_t bx) {
    constexpr int kWhich = SEGS == 1 ? BT_CAP4 : BT_CAP8;   // SEGS segments per wave
    const int t = task(w, kWhich, (int)bx);
    SelState* st = w.st + t;
    PASS_STAMP(1, 0);
    if (!st->lower_pending) return;
    PASS_STAMP(1, 1);
    const TDesc d = w.td[t];   // by value: stores below cannot alias it
    const float* vec = vec_flat + d.off;
    const int m = p.max_iters;
    float th[kMaxLower + 1];
    th[0] = st->t_cur;
#pragma unroll
    for (int j = 1; j <= kMaxLower; ++j) th[j] = thr_mul(th[j - 1], p.lower, p.tdtype);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ uint32_t part[kSegPerBlock4][kMaxLower + 1];
    if (lane == 0)
        for (int j = 1; j <= kMaxLower; ++j) part[wave][j] = 0;
    // A wave per segment, its four tiles loaded before the first compare, then the m
    // thresholds one after the other (a uniform loop), each compare a ballot whose
    // popcount the scalar unit adds (per-lane "c[j] += |x| >= t_j" over all 16 slots
    // behind a divergent |x| >= t_m branch kept the VALU busy ~5 us per workgroup after
    // its loads: tools/pass_prof.py). Four segments per wave (a quarter of the
    // workgroups — 6227 of them take 10 us to dispatch) was slower either way: 22 us per
    // workgroup with per-lane counts, 16 with these.
    const int64_t nb = w.bt[kWhich][t + 1] - w.bt[kWhich][t];
    const int64_t nsup = ceil_div(d.nseg, (int64_t)SEGS);
    constexpr int kT = SEGS * kSegTiles;
    for (int64_t su = (bx - w.bt[kWhich][t]) * kSegPerBlock4 + wave; su < nsup; su += nb * kSegPerBlock4) {
        float xs[kT][4];
        uint32_t vs[kT];
#pragma unroll
        for (int u = 0; u < kT; ++u) load_tile<ALIGNED>(vec, d.n, su * (SEGS * kSeg) + u * 256 + 4 * lane, xs[u], vs[u]);
#pragma unroll
        for (int u = 0; u < kT; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q) xs[u][q] = ((vs[u] >> q) & 1u) ? fabsf(xs[u][q]) : -1.f;   // (NaN: never >=)
        PASS_LOADED(1);
        float tj = th[0];
        for (int j = 1; j <= m; ++j) {   // uniform
            tj = thr_mul(tj, p.lower, p.tdtype);   // = th[j]
            uint32_t cj = 0;
#pragma unroll
            for (int u = 0; u < kT; ++u)
#pragma unroll
                for (int q = 0; q < 4; ++q) cj += (uint32_t)__popcll(__ballot(xs[u][q] >= tj));
            if (lane == 0) part[wave][j] += cj;
        }
    }
    __syncthreads();
    PASS_STAMP(1, 2);
    if (threadIdx.x >= 1 && threadIdx.x <= m) {
        const int j = threadIdx.x;
        const uint64_t v = (uint64_t)part[0][j] + part[1][j] + part[2][j] + part[3][j];
        if (v) atomicAdd(&st->lower_cnt[j], (unsigned long long)v);
    }
    PASS_STAMP(1, 3);
    if (!last_block_arrival(&st->tickets[0], (uint32_t)nb)) return;
    if (threadIdx.x < kWave) {
        // the m counts loaded together, one lane each (a loop of dependent agent-scope
        // loads paid an L2 round trip per threshold); j* = the first reaching lower*k
        const int j = lane + 1;
        const bool hit = j <= m && (long long)load_count(&st->lower_cnt[j]) >= d.lower_count;
        const uint64_t hb = __ballot(hit);
        const int js = hb ? __builtin_ctzll(hb) + 1 : m;
        if (threadIdx.x == 0) {
        st->t_cur = th[js];
        st->iter = js;
        st->recounts = js;
        st->overflow = 0;
        st->lower_pending = 0;
        st->active = 1;   // count pass + decide at t_{j*}
        }
    }
    PASS_STAMP(1, 4);
}

template <bool ALIGNED, int SEGS>
__global__ void __launch_bounds__(kBlock)
k_lower_counts(const float* __restrict__ vec_flat, SelWS w, SelCfg p) {
    lower_counts_body<ALIGNED, SEGS>(vec_flat, w, p, blockIdx.x);
}

// The "lower" recounts served by the K1 candidate lists: the counts at the first
// kLowerLists thresholds t_j that are >= t_list, from the complete lists (a spilled
// segment is re-read by a wave). When one of them reaches lower*k, the first such j
// is the reference's j* and k_lower_counts' pass over vec is skipped; otherwise the
// counts are cleared and k_lower_counts recounts every t_j over vec. One thread per
// segment, like k_count_lists.
constexpr int kLowerLists = 4;

__device__ __forceinline__ void lower_lists_body(const float* __restrict__ vec_flat, const SelWS& w, const SelCfg& p,
                                                 int64_t bx) {
    const int t = task(w, BT_SEG, (int)bx);
    SelState* st = w.st + t;
    if (!st->lower_pending) return;
    float th[kLowerLists + 1];
    th[0] = st->t_cur;
#pragma unroll
    for (int j = 1; j <= kLowerLists; ++j) th[j] = thr_mul(th[j - 1], p.lower, p.tdtype);
    const float tl = st->t_list;
    int ms = 0;   // thresholds t_1..t_ms are served by the lists (uniform per tensor)
#pragma unroll
    for (int j = 1; j <= kLowerLists; ++j)
        if (j <= p.max_iters && th[j] >= tl) ms = j;
    if (ms == 0) return;
    const TDesc d = w.td[t];   // by value: stores below cannot alias it
    const float* vec = vec_flat + d.off;
    __shared__ int spill[kBlock];
    __shared__ int nspill;
    __shared__ uint32_t bsum[kLowerLists + 1];
    if (threadIdx.x == 0) nspill = 0;
    if (threadIdx.x <= kLowerLists) bsum[threadIdx.x] = 0;
    __syncthreads();
    const int64_t lseg0 = (bx - w.bt[BT_SEG][t]) * kBlock;
    const int64_t ls = lseg0 + threadIdx.x;
    uint32_t c[kLowerLists + 1];
#pragma unroll
    for (int j = 0; j <= kLowerLists; ++j) c[j] = 0;
    if (ls < d.nseg) {
        const int64_t seg = d.seg0 + ls;
        const uint32_t lc = lcnt_count(w.seg_lcnt[seg]);
        if (lc <= (uint32_t)kCap) {
            for (uint32_t e0 = 0; e0 < lc; e0 += 16) {   // 16 loads in flight at a time
                float v[16];
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    if (e0 + q < lc) v[q] = w.lst_val[lslot(seg, e0 + q)];
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    if (e0 + q < lc) {
                        const float a = fabsf(v[q]);
#pragma unroll
                        for (int j = 1; j <= kLowerLists; ++j) c[j] += (j <= ms) && a >= th[j];
                    }
            }
        } else {
            spill[atomicAdd(&nspill, 1)] = threadIdx.x;
        }
    }
#pragma unroll
    for (int j = 1; j <= kLowerLists; ++j) {
        const uint32_t v = wave_sum(c[j]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&bsum[j], v);
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    for (int q = wave; q < nspill; q += kSegPerBlock4) {
        float x[kSegTiles][4];
        uint32_t valid[kSegTiles];
        load_segment(vec, d.n, lseg0 + spill[q], x, valid);
        for (int j = 1; j <= ms; ++j) {
            uint32_t cs = 0;
#pragma unroll
            for (int u = 0; u < kSegTiles; ++u) cs += __popc(ge_mask(x[u], valid[u], th[j]));
            cs = wave_sum(cs);
            if ((threadIdx.x & 63) == 0 && cs) atomicAdd(&bsum[j], cs);
        }
    }
    __syncthreads();
    if (threadIdx.x >= 1 && threadIdx.x <= ms && bsum[threadIdx.x])
        atomicAdd(&st->lower_cnt[threadIdx.x], (unsigned long long)bsum[threadIdx.x]);
    const uint32_t nb = (uint32_t)(w.bt[BT_SEG][t + 1] - w.bt[BT_SEG][t]);
    if (!last_block_arrival(&st->tickets[2], nb)) return;
    if (threadIdx.x < kWave) {
        // the ms counts loaded together, one lane each (see k_lower_counts)
        const int jl = (int)(threadIdx.x & 63) + 1;
        const bool hit = jl <= ms && (long long)load_count(&st->lower_cnt[jl]) >= d.lower_count;
        const uint64_t hb = __ballot(hit);
        int js = hb ? __builtin_ctzll(hb) + 1 : 0;
        if (threadIdx.x == 0) {
        // every t_j served and none reaches lower*k: t_(max_iters), as k_lower_counts picks
        if (!js && ms == p.max_iters) js = ms;
        if (js) {
            st->t_cur = th[js];
            st->iter = js;
            st->recounts = js;
            st->overflow = 0;
            st->lower_pending = 0;
            st->active = 1;   // count pass + decide at t_{j*}
        } else {
            for (int j = 1; j <= ms; ++j) st->lower_cnt[j] = 0;   // k_lower_counts recounts every t_j
        }
        }
    }
}

__global__ void __launch_bounds__(kBlock)
k_lower_lists(const float* __restrict__ vec_flat, SelWS w, SelCfg p) {
    lower_lists_body(vec_flat, w, p, blockIdx.x);
}
}  // namespace dgc
