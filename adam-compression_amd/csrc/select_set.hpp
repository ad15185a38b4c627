// Selection, K5s: an untied resample's set emitted in index order by co-resident
// workgroups (resample_set_block, k_resample_set). The one declared cross-stage edge:
// resample_set_block is declared in select_emit.hpp, whose k_emit_wide_t<true> runs it
// in the emit's launch, and defined here. Relies on select_emit.hpp (EmitOut, out_base,
// emit_one), radix_select.hpp (kScanThreads) and introselect.hpp (the consensus votes).
#pragma once
#include "select_emit.hpp"

namespace dgc {
// For an engine (resample_order = 1) a resampled tensor's payload need not list torch's
// topk order: the exchange's decompress (index_put_ of distinct indices) and
// DGCSGDMemory.update depend on the SET of the top-k (dgc/compression.py:134-137,
// 179-194; dgc/memory.py:72-77). When the k-th largest candidate key is not tied
// across the k boundary (#keys >= kth == k) every top-k is that set, whatever order
// and tie rule produced it, so it is emitted in index order and the exact replay (K5)
// skips the tensor (rs_nth = 3). Tied, the replay runs as always. The k-th largest is
// found by a radix select over key - key(t_cur) (every candidate is >= t_cur) in two
// passes over the kSetSpan = 25 bits above key(t_cur): kSetBins0 = 4096 bins of bits
// 13-24, clamped (the top bin also takes every key past the span; the k-th largest
// there goes to the replay), then kSetBins1 = 8192 bins of bits 0-12 under the first
// pass's prefix; the emit carries the wire casts and the masking of the K5 emit.
//
// Over G co-resident workgroups of ONE launch (the tensor's BT_SET workgroups: kSetGDefault,
// up to kSetGBig for a capacity past kSetGDefault x kSetCoopMin — VGG-16-BN's fc6, where four
// sliced launches k_bigset_* ran as no-ops every step before; one for a capacity up to
// kSetCoopMin, and none for a tensor that cannot resample — a fixed 16 per tensor took
// ~10 us to dispatch): a set of more than kSetCoopMin candidates is cut into G contiguous
// stretches of rounds, each workgroup's keys in its registers; the radix passes'
// histograms and the per-stretch counts go through device atomics with a barrier
// between the phases (pass 0 | pass 1 | counts), and each
// workgroup emits its stretch's selected entries at the count of the stretches before
// it plus their order inside it — the index order, as one workgroup emits it. A set of
// up to kSetRegC x 1024 candidates takes the same code on one workgroup, with no
// barrier. The G workgroups start with a residency consensus (as K5's global phase):
// should they not all be resident within kSetArriveTicks, the tensor is left to the
// exact replay (k_nth_select), exact either way; so is a barrier that times out (not
// expected after the consensus), and a tie across the k boundary as before.
// (ResNet-50's 72k-candidate resample: one workgroup walked its keys six times, 24 of
// 72 rounds from L2 — 59 us of the step.)
constexpr uint64_t kSetArriveTicks = 200000;   // 2 ms of the 100 MHz wall clock
static_assert(kSetCoopMin == (int64_t)kSetRegC * kScanThreads, "K5s: one workgroup holds kSetCoopMin keys");

__device__ __forceinline__ bool setg_consensus(SetG* g, uint32_t G) {
    __shared__ uint32_t verdict;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t a = __hip_atomic_fetch_add(&g->arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (a + 1 == G) {
            atomicCAS(&g->decide, (uint32_t)kNthGUndecided, (uint32_t)kNthGGo);
        } else {
            const uint64_t t0 = wall_clock64();
            while (__hip_atomic_load(&g->decide, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kNthGUndecided) {
                if (wall_clock64() - t0 > kSetArriveTicks) {
                    atomicCAS(&g->decide, (uint32_t)kNthGUndecided, (uint32_t)kNthGAbort);
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
        }
        verdict = __hip_atomic_load(&g->decide, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    return verdict == kNthGGo;
}

// Barrier among the G workgroups: everything they exchange is device atomics, read back
// with agent-scope atomic loads (last_block_arrival's "atomics both sides"), so draining
// this workgroup's atomics (vmcnt(0)) before the arrival is the only ordering needed.
__device__ __forceinline__ void setg_barrier(SetG* g, uint32_t G, uint32_t* status) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t gen = __hip_atomic_load(&g->bar_gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t a = __hip_atomic_fetch_add(&g->bar_count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (a == G - 1) {
            __hip_atomic_store(&g->bar_count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_fetch_add(&g->bar_gen, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            bool passed = false;
            for (uint32_t spin = 0; spin < (1u << 24); ++spin) {
                if (__hip_atomic_load(&g->bar_gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != gen) {
                    passed = true;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            if (!passed) {   // the replay takes the tensor (exact); recorded for the caller
                __hip_atomic_store(&g->broken, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                atomicOr(status, (uint32_t)DGC_K5_SET_BROKEN);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
}

// (OVF: a stretch longer than the registers hold — a set above ~2M candidates; the
// common case compiles without the L2 rounds)
template <bool OVF>
__device__ __forceinline__ void resample_set_body(const float* __restrict__ vec_flat, const SelWS& w, const EmitOut& o,
                                                  int t, uint32_t b, uint32_t G, int per, int rounds,
                                                  SelState* st, const TDesc& d) {
    const int64_t n64 = st->n_cur;
    SetG* g = w.setg + t;
    if (G > 1 && !setg_consensus(g, G)) {   // not all resident: the replay (recorded for the caller)
        if (b == 0 && threadIdx.x == 0) atomicOr(&w.nthg[t].status, (uint32_t)DGC_K5_SET_FALLBACK);
        return;
    }
    SET_STAMP(0);
    const int n = (int)n64;
    const uint32_t k = (uint32_t)d.k;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    constexpr int kWaves = kScanThreads / kWave;
    __shared__ uint32_t h[kSetBins1];
    __shared__ uint32_t lds32[16];
    __shared__ uint32_t rbase[(OVF ? kSetRoundsMax : kSetRegC) * kWaves];
    __shared__ uint32_t sel_above, sel_cnt, s_base, s_stop;
    __shared__ int sel_bin;
    __shared__ long long obase_s;
    // this workgroup's stretch of rounds; queue entry i = tid + r * 1024 (coalesced)
    const int r0 = (int)b * per, r1 = min(r0 + per, rounds);
    const DGC_GLB uint32_t* qk = glb(w.cand_key + d.cand_off);
    auto valid = [&](int r) { return r0 + r < r1 && tid + (r0 + r) * kScanThreads < n; };
    uint32_t key[kSetRegC];
#pragma unroll
    for (int r = 0; r < kSetRegC; ++r) key[r] = valid(r) ? qk[tid + (r0 + r) * kScanThreads] : 0u;
    // every round of the stretch: the registers, then (a big set only) the rest from L2
    auto walk = [&](auto&& f) {
#pragma unroll
        for (int r = 0; r < kSetRegC; ++r) f(r, key[r], valid(r));
        if (OVF)
            for (int r = kSetRegC; r < per; ++r) {
                const bool v = valid(r);
                f(r, v ? qk[tid + (r0 + r) * kScanThreads] : 0u, v);
            }
    };
    // the key range: every candidate has |x| >= t_cur (the gather's test), so key(t_cur)
    // bounds it from below, and the two passes cover kSetSpan bits above it (4 octaves):
    // the first pass's top bin also takes every key past that span, and should the k-th
    // largest fall there the replay takes the tensor (exact either way). Two passes of
    // 4096 and 8192 bins, not three of 2048: each pass of a cooperative set is a merge
    // and a barrier (~5 us over 16 workgroups). A min/max phase over the keys cost a
    // barrier too (2.2 us in one workgroup, 5.5 us over 16); an open range up to
    // 0x7FFFFFFF piled the first pass into a few bins (LDS atomics on the same words:
    // +8 us in one workgroup, tools/k5s_prof.py).
    const uint32_t mn = abs_key(st->t_cur);
    for (int q = tid; q < kSetBins1; q += kScanThreads) h[q] = 0;
    __syncthreads();
    SET_STAMP(1);
    static_assert(kSetBins0 == 4 * kScanThreads && kSetBins1 == 8 * kScanThreads, "pick_bin_small<4 | 8>");
    int passes = 0;   // (whose merged histograms this workgroup re-zeroes its share of)
    uint32_t prefix = 0, k_rem = k;
    uint32_t kth = mn, eq = (uint32_t)n;
    bool ok = true;
    for (int pass = 0; pass < 2; ++pass) {
        const uint32_t nb = pass == 0 ? (uint32_t)kSetBins0 : (uint32_t)kSetBins1;
        walk([&](int, uint32_t kk, bool v) {
            const uint32_t x = kk - mn;
            if (!v) return;
            if (pass == 0) atomicAdd(&h[min(x >> kSetLo0, nb - 1u)], 1u);
            else if ((x >> kSetLo0) == prefix) atomicAdd(&h[x & (nb - 1u)], 1u);
        });
        __syncthreads();
        if (G > 1) {   // every workgroup picks the same bin from the same merged histogram
            uint32_t* gh = pass == 0 ? g->hist0 : g->hist1;
            for (int q = tid; q < (int)nb; q += kScanThreads)
                if (h[q]) __hip_atomic_fetch_add(&gh[q], h[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            setg_barrier(g, G, &w.nthg[t].status);
            for (int q = tid; q < (int)nb; q += kScanThreads)
                h[q] = __hip_atomic_load(&gh[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
        }
        if (tid == 0) sel_bin = -1;
        __syncthreads();
        int bin;
        uint32_t above;
        const bool hit = pass == 0 ? pick_bin_small<4>(h, k_rem, lds32, &bin, &above)
                                   : pick_bin_small<8>(h, k_rem, lds32, &bin, &above);
        if (hit) {
            sel_bin = bin;
            sel_above = above;
            sel_cnt = h[bin];
        }
        __syncthreads();
        const int sb = sel_bin;
        const uint32_t a = sel_above, c = sel_cnt;
        __syncthreads();   // every thread has read sel_*
        for (int q = tid; q < (int)nb; q += kScanThreads) h[q] = 0;
        __syncthreads();   // zeroed before the next pass's adds (a wave ahead lost counts to a late zero)
        passes = pass + 1;
        if (sb < 0 || (pass == 0 && sb == kSetBins0 - 1)) {   // (sb < 0 cannot happen: k < n keys)
            ok = false;   // the k-th largest is 4 octaves or more above t_cur: the replay takes it
            break;
        }
        k_rem -= a;
        if (pass == 0) {
            prefix = (uint32_t)sb;
        } else {
            kth = mn + ((prefix << kSetLo0) | (uint32_t)sb);
            eq = c;
        }
    }
    __syncthreads();
    // tied across the boundary (more keys == kth than the k - #(> kth) still needed):
    // only torch's exact order of operations knows which ones — the replay
    if (eq != k_rem) ok = false;
    SET_STAMP(2);
    // order-preserving compaction: (round, wave) ballot counts, one workgroup scan, the
    // stretches before this one (their counts through the last barrier)
    walk([&](int r, uint32_t kk, bool v) {
        const uint32_t c = ok ? (uint32_t)__popcll(__ballot(v && kk >= kth)) : 0u;
        if (lane == 0) rbase[r * kWaves + wv] = c;
    });
    __syncthreads();
    {
        const uint32_t c = tid < per * kWaves ? rbase[tid] : 0u;
        uint32_t total;
        const uint32_t run = block_exclusive_scan32(c, lds32, &total);
        if (tid < per * kWaves) rbase[tid] = run;
        if (tid == 0) {
            s_base = 0;
            s_stop = ok ? 0u : 1u;
            if (G > 1) __hip_atomic_store(&g->cnt[b], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    static_assert(kSetRoundsMax * kWaves <= kScanThreads, "one compaction count per thread");
    if (G > 1) {
        setg_barrier(g, G, &w.nthg[t].status);
        if (tid == 0) {
            uint32_t base = 0;
            for (uint32_t i = 0; i < b; ++i)
                base += __hip_atomic_load(&g->cnt[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_base = base;
            if (__hip_atomic_load(&g->broken, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) s_stop = 1;
        }
        // every workgroup has read the histograms: re-zero this one's share of those used
        for (int p = 0; p < passes; ++p) {
            const int nb = p == 0 ? kSetBins0 : kSetBins1, share = (nb + (int)G - 1) / (int)G;
            uint32_t* gh = p == 0 ? g->hist0 : g->hist1;
            const int qlo = (int)b * share, qhi = min(qlo + share, nb);
            for (int q = qlo + tid; q < qhi; q += kScanThreads) gh[q] = 0;
        }
    }
    if (wv == 0) {
        const long long ob = out_base(w, t);
        if (lane == 0) obase_s = ob;
    }
    __syncthreads();
    if (s_stop) return;   // uniform: a tie or a broken barrier — the replay takes the tensor
    SET_STAMP(3);
    const long long ob = obase_s + (long long)s_base;
    const int64_t* cand = w.cand_idx + d.cand_off;
    const float* cval = w.cand_val + d.cand_off;
    // the register rounds 8 at a time, every selected candidate's index and value loaded
    // before the first store (the stores may alias the loads, so a round-by-round walk
    // waited out a load round trip per round: 12 us for 16k candidates in one workgroup)
    constexpr int kEmitRounds = 8;
    static_assert(kSetRegC % kEmitRounds == 0, "emit batches");
#pragma unroll
    for (int r0b = 0; r0b < kSetRegC; r0b += kEmitRounds) {
        int64_t ci[kEmitRounds];
        float cv[kEmitRounds];
        bool sl[kEmitRounds];
#pragma unroll
        for (int j = 0; j < kEmitRounds; ++j) {
            const int r = r0b + j;
            sl[j] = valid(r) && key[r] >= kth;
            const int i = tid + (r0 + r) * kScanThreads;
            ci[j] = sl[j] ? cand[i] : 0;
            cv[j] = sl[j] ? cval[i] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < kEmitRounds; ++j) {
            const uint64_t mm = __ballot(sl[j]);
            if (sl[j]) emit_one(o, d, ob + rbase[(r0b + j) * kWaves + wv] + mbcnt64(mm, 0u), ci[j], cv[j]);
        }
    }
    if (OVF)
        for (int r = kSetRegC; r < per; ++r) {
            const int i = tid + (r0 + r) * kScanThreads;
            const bool sel = valid(r) && qk[i] >= kth;
            const uint64_t mm = __ballot(sel);
            if (sel) emit_one(o, d, ob + rbase[r * kWaves + wv] + mbcnt64(mm, 0u), cand[i], cval[i]);
        }
    if (b == 0 && tid == 0) {
        st->rs_nth = 3;   // K5's replay and emit skip the tensor
        st->tie_rule = DGC_TIES_SET;
    }
    SET_STAMP(4);
}

// One workgroup of k_resample_set (bx: its index in the BT_SET grid). wait: k_emit_set,
// whose emit workgroups gather the candidates in the same launch — the set's workgroups
// first wait until all of the tensor's emit workgroups have counted themselves (bounded:
// past kSetArriveTicks the tensor is left to the exact replay, recorded as a fallback).
__device__ __forceinline__ void resample_set_block(const float* __restrict__ vec_flat, const SelWS& w,
                                                   const EmitOut& o, int bx, bool wait) {
    const int t = task(w, BT_SET, bx);
    const uint32_t b = (uint32_t)bx - (uint32_t)w.bt[BT_SET][t];
    SelState* st = w.st + t;
    if (st->branch != DGC_BRANCH_RESAMPLE || st->rs_nth != 1) return;   // uniform per workgroup
    const TDesc d = w.td[t];   // by value: stores below cannot alias it
    const uint32_t Gt = (uint32_t)(w.bt[BT_SET][t + 1] - w.bt[BT_SET][t]);   // this tensor's workgroups
    const int64_t n64 = st->n_cur;
    if (d.k < 1 || n64 <= d.k) return;
    // this set's workgroups: one up to kSetCoopMin candidates, else kSetGDefault, and for a big
    // tensor as many as keep its stretches in registers (up to Gt); each stretch's rounds
    // past the registers are read from L2 on every walk, up to kSetRoundsMax per stretch
    const int rounds = (int)((n64 + kScanThreads - 1) / kScanThreads);
    uint32_t G = 1;
    constexpr uint32_t gmin = kSetGDefault;
    if (n64 > kSetOneMax && Gt > 1) {   // (then Gt >= gmin: n64 <= cand_cap)
        const uint32_t want = (uint32_t)((rounds + kSetRegC - 1) / kSetRegC);
        G = want > gmin ? (want < Gt ? want : Gt) : gmin;
        G = G < Gt ? G : Gt;
    }
    const int per = (rounds + (int)G - 1) / (int)G;
    if (per > kSetRoundsMax || b >= G) return;   // (past kSetRoundsMax: the replay)
    if (wait) {
        __shared__ int gathered;
        if (threadIdx.x == 0) {
            const uint32_t want = (uint32_t)(w.bt[BT_GRP][t + 1] - w.bt[BT_GRP][t]);
            const uint64_t t0 = wall_clock64();
            bool ok = true;
            while (__hip_atomic_load(&w.setg[t].gathered, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
                if (wall_clock64() - t0 > kSetArriveTicks) {
                    ok = false;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            if (!ok) atomicOr(&w.nthg[t].status, (uint32_t)DGC_K5_SET_FALLBACK);
            gathered = ok;
        }
        __syncthreads();
        ES_STAMP(1);
        // (a cooperative set's other workgroups then fail the residency consensus: the replay)
        if (!gathered) return;
    }
    if (per > kSetRegC)
        resample_set_body<true>(vec_flat, w, o, t, b, G, per, rounds, st, d);
    else
        resample_set_body<false>(vec_flat, w, o, t, b, G, per, rounds, st, d);
}

__global__ void __launch_bounds__(kScanThreads)
k_resample_set(const float* __restrict__ vec_flat, SelWS w, EmitOut o) {
    resample_set_block(vec_flat, w, o, (int)blockIdx.x, false);
}
}  // namespace dgc
