// Selection, emit: EmitOut, out_base and emit_one (every payload writer's, the resample
// headers' too), k_emit, k_chain_one, the wide emit (k_emit_wide_t; with the sets:
// k_emit_set), the count-emit with its look-back, FinishArgs / sel_finish_body /
// k_sel_finish, and k_emit_queue. Relies on select_count.hpp (the *_body passes, the
// stamps) and select_state.hpp (decide_tensor). The one declared cross-stage edge:
// resample_set_block is declared here and defined in select_set.hpp.
#pragma once
#include "select_count.hpp"

namespace dgc {
struct EmitOut {
    float* vec;          // flat; null: leave vec untouched (pure selection)
    float* mmt;          // flat; null: no momentum masking
    void* values;
    void* indices;
    int32_t vdtype, idtype;
    uint64_t* queue;     // non-null: K5 candidate gather (queue[pos] = key << 32 | pos, cand[pos] = index)
    int64_t* cand;
    int32_t defer;       // first-k branches: leave vec/mmt to the next K1 (record seg_off instead)
    float* cval;         // the K5 gather: cval[pos] = the candidate's value (null: not kept)
    uint32_t* ckey;      //   and ckey[pos] = its key
    int32_t no_queue;    // the gather leaves queue[] unwritten (k_nth_select rebuilds it from ckey)
};

// Entries a tensor emits: the first `limit` candidates, or k after a resample.
__device__ __forceinline__ long long final_count(const SelState& s, int64_t k) {
    return s.branch == DGC_BRANCH_RESAMPLE ? (long long)k : s.limit;
}

// Output position of a tensor's first entry: the entries of the tensors before it.
// The payload position of tensor t's first entry: the final counts of the tensors
// before it, summed by one wave (all loads in flight at once — a serial loop over 50
// tensors was 50 dependent round trips). Call from a whole wave; every lane gets it.
__device__ __forceinline__ long long out_base(const SelWS& w, int t) {
    long long b = 0;
    for (int u0 = 0; u0 < t; u0 += kWave) {
        const int u = u0 + (int)(threadIdx.x & 63);
        b += u < t ? final_count(w.st[u], w.td[u].k) : 0;
    }
    return wave_sum(b);
}

// pos: output slot; li: the element's index within its tensor (d.off + li in the flat buffers).
__device__ __forceinline__ void emit_one(const EmitOut& o, const TDesc& d, long long pos, int64_t li, float x,
                                         bool mask_now = true) {
    if (o.queue) {
        if (!o.no_queue) o.queue[d.cand_off + pos] = ((uint64_t)abs_key(x) << 32) | (uint64_t)(uint32_t)pos;
        o.cand[d.cand_off + pos] = li;
        if (o.cval) {
            o.cval[d.cand_off + pos] = x;
            o.ckey[d.cand_off + pos] = abs_key(x);
        }
        return;
    }
    store_value(o.values, pos, x, o.vdtype);
    store_index(o.indices, pos, d.idx_base + li, o.idtype);
    if (!mask_now) return;
    // scattered 4-B writes, one per 128-B line: non-temporal (no L2 allocation)
    if (o.vec) __builtin_nontemporal_store(0.f, o.vec + d.off + li);
    if (o.mmt) __builtin_nontemporal_store(0.f, o.mmt + d.off + li);
}

// Wave-cooperative emit of one spilled segment (local ls) from its elements in
// registers (xs / vs: load_segment's).
// FIRSTK: positions base + rank for |x| >= t, kept while < limit.
__device__ __forceinline__ void emit_segment_firstk(const float (&xs)[kSegTiles][4], const uint32_t (&vs)[kSegTiles],
                                                    const TDesc& d, int64_t ls, long long base, long long limit,
                                                    long long obase, float t, const EmitOut& o, bool mask_now) {
    const int lane = threadIdx.x & 63;
    uint32_t run = 0;
#pragma unroll
    for (int tile = 0; tile < kSegTiles; ++tile) {
        const float(&x)[4] = xs[tile];
        const int64_t e0 = ls * kSeg + tile * 256 + 4 * lane;
        const uint32_t pm = ge_mask(x, vs[tile], t);
        if (__ballot(pm != 0)) {
            uint32_t lb, tot;
            wave_prefix4(pm, lb, tot);
            uint32_t r = run + lb;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (pm & (1u << j)) {
                    const long long pos = base + r;
                    if (pos < limit) emit_one(o, d, obase + pos, e0 + j, x[j], mask_now);
                    ++r;
                }
            run += tot;
        }
    }
}

// ... re-reading vec. (Two segments per call with both loads in flight made no
// difference to ResNet-50's emit, whose spilled small tensors end ~17 us into the launch:
// tools/es_prof.py.)
__device__ __forceinline__ void emit_reread_firstk(const float* __restrict__ vec, const TDesc& d, int64_t ls,
                                                   long long base, long long limit, long long obase, float t,
                                                   const EmitOut& o, bool mask_now) {
    float xs[kSegTiles][4];
    uint32_t vs[kSegTiles];
    load_segment(vec, d.n, ls, xs, vs);
    emit_segment_firstk(xs, vs, d, ls, base, limit, obase, t, o, mask_now);
}

// kEmitSplit workgroups of kEmitSegs threads per group of kGroupSegs segments, one
// thread per segment of its quarter. In-group offsets: the quarter's exclusive scan
// plus the counts of the group's earlier quarters (read by the same threads, packed
// into the high half of the one 64-bit scan). Then
//   short lists (<= kEmitShort entries, the common case once the list threshold
//   tracks the selection): the thread emits its own segment, sequentially — its list
//   loads go out before the scan;
//   longer lists: wave per segment — kCap == 64 list slots, lane l takes entry l (one
//   coalesced load per list), ballot ranks give the positions, kEmitBatch lists in
//   flight per wave;
//   spilled segments (> kCap entries): one wave re-reads the 1024 elements.
// o.queue == null: the payload (every branch but a K5 resample, which k_emit_queue
// writes). o.queue != null: K5's candidate gather — every element >= t_cur, ascending
// (the reference's `indices` before its resample topk), only when K5 serves the tensor.
constexpr int kEmitSegs = kGroupSegs / kEmitSplit;   // segments per workgroup (a quarter group)
constexpr int kEmitBatch = 16;
constexpr int kEmitShort = 16;                  // lists up to this long: a thread emits its segment
constexpr uint32_t kEmitSkip = 0xFFFFFFFFu;
static_assert(kCap == kWave, "wave-per-list emission needs kCap == wavefront width");

__device__ __forceinline__ void emit_body(const float* __restrict__ vec_flat, const SelWS& w, const EmitOut& oa,
                                          int64_t bx) {
    const int t = task(w, BT_GRP, (int)bx);
    const SelState* st = w.st + t;
    if (st->branch == DGC_BRANCH_RESAMPLE && st->rs_nth == 2) return;   // K5b emits it
    if (st->spec_emitted) return;                                        // k_count_emit did
    const bool k5 = st->branch == DGC_BRANCH_RESAMPLE && st->rs_nth == 1;
    // oa.queue set: the K5 tensors gather their candidates into the queue and the
    // others emit their payload in the same launch; unset: the K5 tensors are skipped
    if (k5 && !oa.queue) return;
    EmitOut o = oa;
    if (!k5) o.queue = nullptr;
    const TDesc d = w.td[t];   // by value: stores below cannot alias it
    // first-k branches of an engine that defers: the next K1 zeroes what this emits
    const bool defer_here = o.defer && !k5 && !d.tail;
    const float* vec = vec_flat + d.off;
    const int64_t lb = bx - w.bt[BT_GRP][t];
    const int64_t lg = lb / kEmitSplit;                      // group within the tensor
    const int sub = (int)(lb % kEmitSplit);                  // its quarter
    const int64_t g = d.grp0 + lg;
    const int64_t lseg0 = lg * kGroupSegs + (int64_t)sub * kEmitSegs;   // first segment of the quarter
    __shared__ uint32_t off_a[kEmitSegs], lcn[kEmitSegs];
    __shared__ uint64_t lds16[16];
    __shared__ long long obase_s;
    if (threadIdx.x < kWave) {
        const long long b = k5 ? 0 : out_base(w, t);
        if (threadIdx.x == 0) obase_s = b;
    }
    const long long limit = k5 ? st->n_cur : st->limit;
    const long long ga = w.grp_off[g];
    const float tc = st->t_cur;
    {
        // thread jq <-> segment jq of the quarter, plus the earlier quarters' counts at
        // the same position
        const int jq = (int)threadIdx.x;
        const int64_t ls = lseg0 + jq;
        uint32_t ca = 0, lc = 0, pa = 0;
        if (ls < d.nseg) {
            const int64_t seg = d.seg0 + ls;
            ca = w.seg_cnt[seg];
            lc = lcnt_count(w.seg_lcnt[seg]);
        }
#pragma unroll
        for (int q = 0; q < kEmitSplit - 1; ++q) {   // the same position in the group's earlier
            if (q < sub) {                             // quarters (loads in flight together)
                const int64_t seg = d.seg0 + lg * kGroupSegs + (int64_t)q * kEmitSegs + threadIdx.x;
                pa += w.seg_cnt[seg];
            }
        }
        // (a list with nothing at the current threshold is not read: most of them at 1e-4)
        const bool short_list = ls < d.nseg && ca > 0 && lc <= (uint32_t)kEmitShort;
        float v[kEmitShort];
        uint16_t e[kEmitShort];
        if (short_list) {
#pragma unroll
            for (int q = 0; q < kEmitShort; ++q)
                if ((uint32_t)q < lc) {
                    v[q] = w.lst_val[lslot(d.seg0 + ls, q)];
                    e[q] = w.lst_off[lslot(d.seg0 + ls, q)];
                }
        }
        // (earlier quarters' total << 32) | this quarter's counts: one scan gives both
        uint64_t tot;
        const uint64_t ra = block_exclusive_scan(((uint64_t)pa << 32) | ca, lds16, &tot);
        const uint32_t oa = (uint32_t)(tot >> 32) + (uint32_t)ra;
        const bool work = ca > 0 && ga + oa < limit;
        if (defer_here && ls < d.nseg) w.seg_off[d.seg0 + ls] = oa;
        off_a[jq] = oa;
        lcn[jq] = (work && !short_list) ? lc : kEmitSkip;
        __syncthreads();   // obase_s
        if (work && short_list) {   // the first `limit` entries >= tc, in index order
            const long long ob0 = obase_s;
            long long pos = ga + oa;
#pragma unroll
            for (int j = 0; j < kEmitShort; ++j)
                if ((uint32_t)j < lc && fabsf(v[j]) >= tc) {
                    if (pos < limit) emit_one(o, d, ob0 + pos, ls * kSeg + e[j], v[j], !defer_here);
                    ++pos;
                }
        }
    }
    __syncthreads();
    const long long obase = obase_s;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t lt = lanemask_lt();
    // which of the wave's segments are left to it (longer lists) and which spilled:
    // one LDS read and two ballots, so a wave with nothing left skips
    constexpr int kWaveSegs = kEmitSegs / (kEmitSegs / kWave);   // 64: one ballot covers them
    const int jw = wv * kWaveSegs;
    const uint32_t Lme = lane < kWaveSegs ? lcn[jw + lane] : kEmitSkip;
    uint64_t todo = __ballot(Lme != kEmitSkip && Lme <= (uint32_t)kCap);
    uint64_t spilled = __ballot(Lme != kEmitSkip && Lme > (uint32_t)kCap);
    for (int b0 = 0; b0 < kWaveSegs; b0 += kEmitBatch) {
        if (!((todo >> b0) & ((1ull << kEmitBatch) - 1))) continue;   // nothing in this batch
        const int j0 = jw + b0;
        float x[kEmitBatch];
        uint32_t e[kEmitBatch];
#pragma unroll
        for (int q = 0; q < kEmitBatch; ++q) {   // all list loads issued first
            const uint32_t L = lcn[j0 + q];
            x[q] = 0.f;
            e[q] = 0;
            if (L <= (uint32_t)kCap && (uint32_t)lane < L) {
                const int64_t slot = lslot(d.seg0 + lseg0 + j0 + q, lane);
                x[q] = w.lst_val[slot];
                e[q] = w.lst_off[slot];
            }
        }
#pragma unroll
        for (int q = 0; q < kEmitBatch; ++q) {
            const uint32_t L = lcn[j0 + q];
            if (L == kEmitSkip || L > (uint32_t)kCap) continue;
            const int64_t ls = lseg0 + j0 + q;
            const long long ba = ga + off_a[j0 + q];
            const bool sel = (uint32_t)lane < L && fabsf(x[q]) >= tc;
            const uint64_t m = __ballot(sel);
            const long long pos = ba + __popcll(m & lt);
            if (sel && pos < limit) emit_one(o, d, obase + pos, ls * kSeg + e[q], x[q], !defer_here);
        }
    }
    while (spilled) {   // rare: one wave re-reads the segment's 1024 elements
        const int j = jw + __builtin_ctzll(spilled);
        spilled &= spilled - 1;
        emit_reread_firstk(vec, d, lseg0 + j, ga + off_a[j], limit, obase, tc, o, !defer_here);
    }
}

__global__ void __launch_bounds__(kEmitSegs)
k_emit(const float* __restrict__ vec_flat, SelWS w, EmitOut oa) {
    emit_body(vec_flat, w, oa, blockIdx.x);
}

// One-tensor DGC_SYNC_DEVICE selections with the lowering shortcut (the flat bucket):
// the lowering from the lists, the lowering over vec and the count at the lowered
// threshold from the lists — three launches that are gated no-ops in the steady state —
// in ONE launch. The two full select passes and the emit stay launches of their own:
// chained, their HBM-bound bodies ran at the combined kernel's 2 waves per SIMD
// (177 VGPRs) and a step whose lists missed took 0.43 ms longer (flat-1B, same box). When
// every tensor is decided (the steady state: the first count's decide) every workgroup
// returns at once. Otherwise the phases run in order
// over virtual blocks that workgroups claim from an atomic counter; each phase's gate is
// decided once, by the first workgroup to reach it, from the state the phases before
// left; a workgroup waits for a phase's completion count (chain_phase_end: one L2
// write-back per XCD that wrote, an acquire per workgroup) before the next phase. Only
// running workgroups claim blocks, so nothing assumes the grid co-resident.
constexpr int kChainPhases = 3;
enum { CH_CLAIM = 0, CH_GATE = kChainPhases };   // words of the first line; then a ChainPhase each
static_assert(32 + kChainPhases * 32 <= kChainOneWords, "SelWS::chain words");

template <bool ALIGNED>
__global__ void __launch_bounds__(kBlock)
k_chain_one(const float* __restrict__ vec_flat, SelWS w, SelCfg p) {
    uint32_t* cc = w.chain;
    __shared__ uint32_t s_u;
    bool open = false;   // a tensor still adapting (every phase below gates on that)
    for (int t = threadIdx.x; !open && t < w.T; t += blockDim.x) open = !w.st[t].done;
    if (!__syncthreads_or(open)) return;   // uniform: the steady state
    for (int ph = 0; ph < kChainPhases; ++ph) {
        // does any tensor need the phase
        bool any = false;
        for (int t = threadIdx.x; !any && t < w.T; t += blockDim.x) {
            const SelState& u = w.st[t];
            any = ph < 2 ? u.lower_pending != 0 : (u.active && u.t_cur >= u.t_list);
        }
        any = __syncthreads_or(any);   // (also: s_u is free again)
        if (threadIdx.x == 0) {
            uint32_t gate = __hip_atomic_load(&cc[CH_GATE + ph], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (gate == 0) {
                const uint32_t want = any ? 2u : 1u;
                const uint32_t prev = atomicCAS(&cc[CH_GATE + ph], 0u, want);
                gate = prev == 0u ? want : prev;
            }
            s_u = gate;
        }
        __syncthreads();
        if (s_u != 2u) continue;   // uniform
        const int which = ph == 0 ? BT_SEG : ph == 1 ? BT_CAP4 : BT_CNT;
        const uint32_t nvb = (uint32_t)w.bt[which][w.T];
        uint32_t mine = 0;
        for (;;) {
            __syncthreads();
            if (threadIdx.x == 0) s_u = atomicAdd(&cc[CH_CLAIM + ph], 1u);
            __syncthreads();
            const uint32_t vb = s_u;
            if (vb >= nvb) break;   // uniform
            if (ph == 0) lower_lists_body(vec_flat, w, p, vb);
            else if (ph == 1) lower_counts_body<ALIGNED>(vec_flat, w, p, vb);
            else count_lists_body(vec_flat, w, p, vb);
            ++mine;
        }
        chain_phase_end(reinterpret_cast<ChainPhase*>(cc + 32) + ph, mine, nvb);
    }
}

__device__ __forceinline__ void resample_set_block(const float* __restrict__ vec_flat, const SelWS& w,
                                                   const EmitOut& o, int bx, bool wait);   // K5s: select_set.hpp

// The few groups of a model gradient set: kEmitSplit workgroups of kGroupSegs threads
// per group, each scanning the whole group (thread per segment) and emitting its
// quarter with 16 waves of 16 segments — one list batch per wave, every list by a
// wave. More waves per quarter beat k_emit's short-list threads there (measured on
// ResNet-50: 12 vs 15 us per launch).
//
// SET (k_emit_set): the emit and k_resample_set in ONE launch. The workgroups from ngb
// on are the sets' (resample_set_block); an emit workgroup that gathered a resampled
// tensor's candidates releases its stores and counts itself in the tensor's
// SetG::gathered, and the tensor's sets start once all of its emit workgroups have —
// beside the other tensors' emit, one launch boundary fewer. The emit workgroups come
// first in the grid and never wait, so a waiting set only holds a slot the emit does
// not need (ResNet-50's whole grid, ~220 workgroups of 1024 threads, is resident at
// once on 256 CUs; VGG-16-BN's ~680 against 512 slots, ~150 of them sets).
// Returns true when the workgroup gathered a resampled tensor's candidates.
__device__ __forceinline__ bool emit_wide_part(const float* __restrict__ vec_flat, const SelWS& w, const EmitOut& oa,
                                               int bx) {
    const int t = task(w, BT_GRP, bx);
    const SelState* st = w.st + t;
    if (st->branch == DGC_BRANCH_RESAMPLE && st->rs_nth == 2) return false;   // K5b emits it
    if (st->spec_emitted) return false;                                        // k_count_emit did
    const bool k5 = st->branch == DGC_BRANCH_RESAMPLE && st->rs_nth == 1;
    // oa.queue set: the K5 tensors gather their candidates into the queue and the
    // others emit their payload in the same launch; unset: the K5 tensors are skipped
    if (k5 && !oa.queue) return false;
    EmitOut o = oa;
    if (!k5) o.queue = nullptr;
    const TDesc d = w.td[t];   // by value: stores below cannot alias it
    // first-k branches of an engine that defers: the next K1 zeroes what this emits
    const bool defer_here = o.defer && !k5 && !d.tail;
    const float* vec = vec_flat + d.off;
    const int64_t lb = (int64_t)bx - w.bt[BT_GRP][t];
    constexpr int split = kEmitSplit;
    const int64_t lg = lb / split;                           // group within the tensor
    const int sub = (int)(lb % split);                       // its share this workgroup emits
    const int64_t g = d.grp0 + lg;
    const int64_t lseg0 = lg * kGroupSegs;
    __shared__ uint32_t off_a[kGroupSegs], lcn[kGroupSegs];
    __shared__ uint64_t lds16[16];
    __shared__ long long obase_s;
    if (threadIdx.x < kWave) {
        const long long b = k5 ? 0 : out_base(w, t);
        if (threadIdx.x == 0) obase_s = b;
    }
    const long long limit = k5 ? st->n_cur : st->limit;
    const long long ga = w.grp_off[g];
    {
        const int64_t ls = lseg0 + threadIdx.x;
        uint32_t ca = 0, lc = 0;
        if (ls < d.nseg) {
            const int64_t seg = d.seg0 + ls;
            ca = w.seg_cnt[seg];
            lc = lcnt_count(w.seg_lcnt[seg]);
        }
        uint64_t tot;
        const uint32_t oa = (uint32_t)block_exclusive_scan((uint64_t)ca, lds16, &tot);
        const bool work = ca > 0 && ga + oa < limit;
        if (defer_here && ls < d.nseg && (int)threadIdx.x / (kGroupSegs / split) == sub)
            w.seg_off[d.seg0 + ls] = oa;
        off_a[threadIdx.x] = oa;
        lcn[threadIdx.x] = work ? lc : kEmitSkip;
    }
    __syncthreads();
    ES_STAMP(1);
    const long long obase = obase_s;
    const float tc = st->t_cur;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t lt = lanemask_lt();
    constexpr int wave_segs = kGroupSegs / split / (kGroupSegs / kWave);
    static_assert(wave_segs % kEmitBatch == 0, "whole batches per wave");
    const int jw = sub * (kGroupSegs / split) + wv * wave_segs;
    for (int j0 = jw; j0 < jw + wave_segs; j0 += kEmitBatch) {
        float x[kEmitBatch];
        uint32_t e[kEmitBatch];
#pragma unroll
        for (int q = 0; q < kEmitBatch; ++q) {   // all list loads issued first
            const uint32_t L = lcn[j0 + q];
            x[q] = 0.f;
            e[q] = 0;
            if (L <= (uint32_t)kCap && (uint32_t)lane < L) {
                const int64_t slot = lslot(d.seg0 + lseg0 + j0 + q, lane);
                x[q] = w.lst_val[slot];
                e[q] = w.lst_off[slot];
            }
        }
        uint32_t spilled = 0;   // (re-read after the batch: a call inside kept the loop rolled)
#pragma unroll
        for (int q = 0; q < kEmitBatch; ++q) {
            const uint32_t L = lcn[j0 + q];
            if (L == kEmitSkip) continue;
            const int64_t ls = lseg0 + j0 + q;
            const long long ba = ga + off_a[j0 + q];
            if (L > (uint32_t)kCap) {
                spilled |= 1u << q;
                continue;
            }
            const bool sel = (uint32_t)lane < L && fabsf(x[q]) >= tc;
            const uint64_t m = __ballot(sel);
            const long long pos = ba + __popcll(m & lt);
            if (sel && pos < limit) emit_one(o, d, obase + pos, ls * kSeg + e[q], x[q], !defer_here);
        }
        while (spilled) {   // rare: the wave re-reads the segment's 1024 elements
            const int q = __builtin_ctz(spilled);
            spilled &= spilled - 1;
            emit_reread_firstk(vec, d, lseg0 + j0 + q, ga + off_a[j0 + q], limit, obase, tc, o, !defer_here);
        }
    }
    return k5;
}

template <bool SET>
__global__ void __launch_bounds__(kGroupSegs)
k_emit_wide_t(const float* __restrict__ vec_flat, SelWS w, EmitOut oa, EmitOut os, int32_t ngb) {
    const int bx = (int)blockIdx.x;
    ES_STAMP(0);
    if (SET && bx >= ngb) {
        resample_set_block(vec_flat, w, os, bx - ngb, true);
    } else if (emit_wide_part(vec_flat, w, oa, bx) && SET) {   // uniform per workgroup
        const int t = task(w, BT_GRP, bx);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            __hip_atomic_fetch_add(&w.setg[t].gathered, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    ES_STAMP(2);
}

// The first count pass of a ONE-tensor call whose lists serve t_cur (the flat
// bucket's steady state), fused with a speculative first-k emit: k_count_lists and
// k_emit read the same list lines one after the other (flat-1B: 32 + 57 us, 7B:
// 112 + 132 us). One workgroup per group, in ticket order; a thread counts four
// consecutive segments, whose list entries e share one 16-B word of a 128-B line.
// The group's offset comes from a decoupled look-back over the earlier groups' words
// (aggregate, then inclusive prefix; a group only waits for groups that took their
// ticket before it, so all of them are running). Every entry >= t_cur at a position
// < k is written: exactly the payload of every first-k branch (ok, trunc, direct,
// exhausted: the first min(count, k)). When decide picks one, spec_emitted makes
// k_emit skip the tensor; otherwise (resample, lower) the later passes emit again
// over it. Host-gated to calls whose emit would not mask (deferred or pure selection)
// and whose payload starts at slot 0 (one tensor).
constexpr unsigned long long kLbAgg = 1ull << 62, kLbPre = 1ull << 63, kLbVal = kLbAgg - 1;
constexpr int kLbSpin = 1 << 22;   // polls (with s_sleep) before a look-back gives up: ~seconds
constexpr int kCeStage = 2048;     // entries a group stages in LDS for coalesced payload writes
#ifdef DGC_K5_PROF
__device__ unsigned long long g_ce_prof[2048][6];   // tools/ce_prof.py: per-group phase stamps
#define CE_STAMP(i) do { if (threadIdx.x == 0 && lg < 2048) g_ce_prof[lg][i] = wall_clock64(); } while (0)
#else
#define CE_STAMP(i) do { } while (0)
#endif

__device__ __forceinline__ void count_emit_body(const float* __restrict__ vec_flat, const SelWS& w, const SelCfg& p,
                                                const EmitOut& o) {
    static_assert(kBlock * kCountSegs == kGroupSegs && kCountSegs == kLstTile, "k_count_emit layout");
    SelState* st = w.st;
    if (!st->active || !(st->t_cur >= st->t_list)) return;
    const TDesc d = w.td[0];   // by value: stores below cannot alias it
    const float* vec = vec_flat + d.off;
    const float tc = st->t_cur;
    const uint32_t tkey = abs_key(tc);
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    __shared__ uint32_t lg_s;
    __shared__ int nspill;
    __shared__ int spill[kGroupSegs];
    __shared__ uint32_t spill_cnt[kGroupSegs];   // a spilled segment's count, then its offset
    __shared__ uint64_t lds16[16];
    __shared__ unsigned long long prefix_s;
    __shared__ float stage_v[kCeStage];
    __shared__ uint32_t stage_i[kCeStage];
    if (tid == 0) {
        lg_s = atomicAdd(&st->ce_ticket, 1u);
        nspill = 0;
    }
    __syncthreads();
    const int64_t lg = lg_s;
    CE_STAMP(0);
    const int64_t ls0 = lg * kGroupSegs + kCountSegs * tid;   // this thread's 4 segments
    const int64_t seg0 = d.seg0 + ls0;                        // a multiple of 4 (one tensor: seg0 = 0)
    uint32_t n[kCountSegs], c[kCountSegs], lc[kCountSegs];
    if (ls0 + 3 < d.nseg) {   // one 16-B load
        const uint4 u = *reinterpret_cast<const uint4*>(w.seg_lcnt + seg0);
        lc[0] = u.x; lc[1] = u.y; lc[2] = u.z; lc[3] = u.w;
    } else {
#pragma unroll
        for (int q = 0; q < kCountSegs; ++q) lc[q] = ls0 + q < d.nseg ? w.seg_lcnt[seg0 + q] : 0u;
    }
#pragma unroll
    for (int q = 0; q < kCountSegs; ++q) {
        n[q] = ((lc[q] >> 16) << 16) <= tkey ? 0u : lcnt_count(lc[q]);   // every |x| < t_cur: nothing
        c[q] = 0;
    }
    uint32_t nmax = 0;   // the longest complete list of the four
#pragma unroll
    for (int q = 0; q < kCountSegs; ++q)
        if (n[q] <= (uint32_t)kCap) nmax = max(nmax, n[q]);
    constexpr int kFirst = 8;   // entries 0..7: the four lists' share of one 128-B line
    const float* lv = w.lst_val;
    const uint16_t* lo = w.lst_off;
    // The emit re-reads the entries (from L2) rather than holding them across the scan
    // and look-back: held, with their offsets, they took the kernel to 145 VGPRs, 3 waves
    // per SIMD, and 768 of flat-1B's 977 groups resident — the rest started up to 90 us
    // late (tools/ce_prof.py); re-read it runs at 103 VGPRs, 4 waves, every group at once.
    float4 a[kFirst];
#pragma unroll
    for (int e = 0; e < kFirst; ++e)
        if ((uint32_t)e < nmax) a[e] = *reinterpret_cast<const float4*>(lv + lslot(seg0, e));
#pragma unroll
    for (int e = 0; e < kFirst; ++e) {
        const float x[4] = {a[e].x, a[e].y, a[e].z, a[e].w};
#pragma unroll
        for (int q = 0; q < kCountSegs; ++q) c[q] += (uint32_t)e < n[q] && n[q] <= (uint32_t)kCap && fabsf(x[q]) >= tc;
    }
    // longer lists, 8 entries in flight at a time: at 1B a list holds ~7 entries at the
    // list threshold, so most threads have one of their four lists past 8, and a loop of
    // one dependent load per entry made this count phase ~37 us of k_count_emit's ~110
    // (tools/ce_prof.py)
    for (uint32_t e0 = kFirst; e0 < nmax; e0 += kFirst) {
        float4 b[kFirst];
#pragma unroll
        for (int e = 0; e < kFirst; ++e)
            if (e0 + e < nmax) b[e] = *reinterpret_cast<const float4*>(lv + lslot(seg0, e0 + e));
#pragma unroll
        for (int e = 0; e < kFirst; ++e) {
            if (e0 + e >= nmax) break;
            const float x[4] = {b[e].x, b[e].y, b[e].z, b[e].w};
#pragma unroll
            for (int q = 0; q < kCountSegs; ++q)
                c[q] += e0 + e < n[q] && n[q] <= (uint32_t)kCap && fabsf(x[q]) >= tc;
        }
    }
#pragma unroll
    for (int q = 0; q < kCountSegs; ++q)
        if (ls0 + q < d.nseg && n[q] > (uint32_t)kCap) spill[atomicAdd(&nspill, 1)] = kCountSegs * tid + q;
    __syncthreads();
    for (int i = wave; i < nspill; i += kBlock / kWave) {   // spilled segments: a wave re-reads each
        const int j = spill[i];
        const uint32_t cs = wave_count_segment(vec, d.n, lg * kGroupSegs + j, tc);
        if (lane == 0) spill_cnt[j] = cs;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kCountSegs; ++q)
        if (ls0 + q < d.nseg && n[q] > (uint32_t)kCap) c[q] = spill_cnt[kCountSegs * tid + q];
    CE_STAMP(1);
    const uint32_t mine = c[0] + c[1] + c[2] + c[3];
    uint64_t total;
    const uint32_t tbase = (uint32_t)block_exclusive_scan((uint64_t)mine, lds16, &total);
    uint32_t off[kCountSegs];
    off[0] = tbase;
#pragma unroll
    for (int q = 1; q < kCountSegs; ++q) off[q] = off[q - 1] + c[q - 1];
#pragma unroll
    for (int q = 0; q < kCountSegs; ++q)
        if (ls0 + q < d.nseg) {
            w.seg_cnt[seg0 + q] = c[q];
            w.seg_off[seg0 + q] = off[q];
            if (n[q] > (uint32_t)kCap) spill_cnt[kCountSegs * tid + q] = off[q];   // now its offset
        }
    // the group's offset: decoupled look-back by wave 0, 64 predecessors per poll (one
    // load each, in flight together: a walk of one load at a time paid ~1 us per group)
    if (wave == 0) {
        unsigned long long* lb = w.grp_lb + d.grp0;
        if (lane == 0) {
            if (total) atomicAdd(&w.grp_cnt[d.grp0 + lg], (unsigned long long)total);
            __hip_atomic_store(&lb[lg], (lg == 0 ? kLbPre : kLbAgg) | total, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
        unsigned long long prefix = 0;
        bool ok = true;
        int64_t j = lg - 1;   // the window's closest predecessor
        int spin = 0;
        while (j >= 0) {
            const int64_t jj = j - lane;
            // before group 0: an inclusive prefix of 0
            const unsigned long long v =
                jj >= 0 ? __hip_atomic_load(&lb[jj], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : kLbPre;
            const uint64_t pre = __ballot((v & kLbPre) != 0), unready = __ballot(v == 0);
            const int first = pre ? __builtin_ctzll(pre) : kWave;   // the closest inclusive prefix
            const uint64_t need = first >= kWave - 1 ? ~0ull : ((2ull << first) - 1);
            if (unready & need) {   // a group in the window has not published yet: poll again
                if (++spin > kLbSpin) {
                    ok = false;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
                continue;
            }
            prefix += wave_sum(lane <= first ? (v & kLbVal) : 0ull);
            if (first < kWave) break;
            j -= kWave;
        }
        if (lane == 0) {
            if (lg > 0 && ok)
                __hip_atomic_store(&lb[lg], kLbPre | (prefix + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!ok) atomicExch(&st->ce_fail, 1);   // no emit from this group: k_emit will run
            prefix_s = ok ? prefix : ~0ull;
        }
    }
    __syncthreads();
    CE_STAMP(2);
    const unsigned long long P = prefix_s;
    const long long limit = d.k;
    // Payload writes one entry per lane in slot order: a group whose entries fit stages
    // them in LDS and copies them out coalesced (written where they fall, a lane per four
    // lists, they were 4- and 8-B stores to 64 lines per instruction: 81 -> 71 us at 1B).
    const bool emit = P != ~0ull && (long long)P < limit;
    const bool staged = emit && nspill == 0 && total <= (uint64_t)kCeStage;
    if (emit) {
        // the entries >= t_cur at positions P + off + rank < k
        for (uint32_t e0 = 0; e0 < nmax; e0 += kFirst) {
            if ((long long)(P + off[0]) >= limit) break;
            uint2 ob[kFirst];
            float4 vb[kFirst];
#pragma unroll
            for (int e = 0; e < kFirst; ++e)
                if (e0 + e < nmax) {
                    ob[e] = *reinterpret_cast<const uint2*>(lo + lslot(seg0, e0 + e));
                    vb[e] = *reinterpret_cast<const float4*>(lv + lslot(seg0, e0 + e));
                }
#pragma unroll
            for (int e = 0; e < kFirst; ++e) {
                if (e0 + e >= nmax) break;
                const float x[4] = {vb[e].x, vb[e].y, vb[e].z, vb[e].w};
                const uint32_t oo[4] = {ob[e].x & 0xFFFFu, ob[e].x >> 16, ob[e].y & 0xFFFFu, ob[e].y >> 16};
#pragma unroll
                for (int q = 0; q < kCountSegs; ++q)
                    if (e0 + e < n[q] && n[q] <= (uint32_t)kCap && fabsf(x[q]) >= tc) {
                        const uint32_t r = off[q];   // in-group slot
                        if (staged) {
                            stage_v[r] = x[q];
                            stage_i[r] = (uint32_t)(kCountSegs * tid + q) * kSeg + oo[q];
                        } else if ((long long)(P + r) < limit) {
                            emit_one(o, d, (long long)(P + r), (ls0 + q) * kSeg + oo[q], x[q], false);
                        }
                        off[q] = r + 1;
                    }
            }
        }
    }
    if (emit && !staged)
        for (int i = wave; i < nspill; i += kBlock / kWave) {   // spilled segments: a wave re-reads each
            const int j = spill[i];
            emit_reread_firstk(vec, d, lg * kGroupSegs + j, (long long)(P + spill_cnt[j]), limit, 0, tc, o, false);
        }
    CE_STAMP(3);
    if (staged) {
        __syncthreads();
        const long long m = std::min<long long>((long long)total, limit - (long long)P);
        const int64_t gbase = lg * kGroupSegs * (int64_t)kSeg;   // the group's first element
        for (long long i = tid; i < m; i += kBlock) {
            store_value(o.values, (long long)P + i, stage_v[i], o.vdtype);
            store_index(o.indices, (long long)P + i, d.idx_base + gbase + stage_i[i], o.idtype);
        }
    }
    CE_STAMP(4);
    // the tensor's last workgroup takes the adaptation step
    if (last_block_arrival8(st->tk8, (uint32_t)lg, (uint32_t)(w.bt[BT_CNT][1] - w.bt[BT_CNT][0])))
        decide_tensor(w, p, 0, 1);
    CE_STAMP(5);
}

__global__ void __launch_bounds__(kBlock)
k_count_emit(const float* __restrict__ vec_flat, SelWS w, SelCfg p, EmitOut o) {
    count_emit_body(vec_flat, w, p, o);
}

// k_count_emit beside the full select pass in ONE launch (one tensor; see k_count_pass):
// the first ncnt workgroups count (and emit) from the lists, the rest re-list over vec
// when the lists do not serve — one of the two does work. The merged kernel keeps the
// select pass's occupancy (its VGPRs bound both; k_count_emit's LDS does not).
template <bool ALIGNED>
__global__ void __launch_bounds__(kBlock)
k_count_emit_pass(const float* __restrict__ vec_flat, SelWS w, SelCfg p, EmitOut o, int which, int ncnt) {
    if ((int)blockIdx.x < ncnt)
        count_emit_body(vec_flat, w, p, o);
    else
        select_pass_body<ALIGNED>(vec_flat, w, which, p, (int64_t)blockIdx.x - ncnt);
}

// Result records; the payload's total count; and every tensor's next speculative
// list threshold, margin x t_cur x growth. One workgroup (any size): k_sel_finish, or
// the last workgroup of k_nth_select.
struct FinishArgs {
    int64_t* count_out;
    dgc_select_info* info;
    float margin;
    int32_t defer, mask_mmt;
    int32_t on;   // k_nth_select: its last workgroup runs the finish (no k_sel_finish launch)
    // Host-mapped (pinned) word of the engine, may be null: a call whose resample replay
    // broke (DGC_K5_BROKEN) stores its status there — a plain system-scope store, only
    // then — so an engine that never synchronises sees it on its next step, for free.
    int32_t* sink;
    uint32_t force;   // DGC_K5_FORCE_BROKEN (tests): status bits added to every resampled tensor
    // may be null: set to DGC_ORDER_ASCENDING when every emitted index of the call is in
    // ascending order (no tensor took the exact replay's topk order), else 0 — the
    // packed payload's header word 1, read by the W = 1 scatter (whole-granule stores)
    int64_t* order_out;
};

__device__ __forceinline__ void sel_finish_body(const SelWS& w, const FinishArgs& f) {
    int64_t* count_out = f.count_out;
    dgc_select_info* info = f.info;
    const float margin = f.margin;
    const int defer = f.defer, mask_mmt = f.mask_mmt;
    __shared__ unsigned long long total;
    __shared__ uint32_t broken, topk_order;
    if (threadIdx.x == 0) {
        total = 0;
        broken = 0;
        topk_order = 0;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < w.T; t += blockDim.x) {
        // every load first, by value (a store through st, info or spec could alias a
        // later load: interleaved they were one dependent memory round trip each, 6.5 us
        // for ResNet-50's 54 tensors), then the stores
        // (the fields it uses, one by one: a copy of the whole state indexed by the epoch
        // gave the finish a 1.2 KB/lane scratch frame — k_nth_select 13 -> 22 us at 1B)
        SelState* st = w.st + t;
        struct {
            float t0, t_cur;
            int32_t branch, recounts, overflow, full_passes, list_spills, epoch, tie_rule, win_keys;
            long long n_cur, limit;
        } s;
        s.t0 = st->t0;
        s.t_cur = st->t_cur;
        s.branch = st->branch;
        s.recounts = st->recounts;
        s.overflow = st->overflow;
        s.full_passes = st->full_passes;
        s.list_spills = st->list_spills;
        s.epoch = st->epoch;
        s.tie_rule = st->tie_rule;
        s.win_keys = st->win_keys;
        s.n_cur = st->n_cur;
        s.limit = st->limit;
        const uint32_t wc = st->win_cnt[s.epoch & 1];   // this call's window, taken or not
        const int64_t k = w.td[t].k;
        const bool tail = w.td[t].tail;
        const uint32_t status = w.nthg[t].status;
        float* spec = w.spec ? w.spec + kSpecWords * t : nullptr;
        const float used = spec ? spec[0] : __builtin_huge_valf();
        const float prev = spec ? spec[1] : __builtin_huge_valf();
        const uint32_t k5 = status | (s.branch == DGC_BRANCH_RESAMPLE ? f.force : 0u);
        if (k5 & DGC_K5_BROKEN) atomicOr(&broken, k5);
        // the exact replays (K5, K5b) emit torch.topk's order; every other branch ascends
        if (s.branch == DGC_BRANCH_RESAMPLE && s.tie_rule == DGC_TIES_EXACT) atomicOr(&topk_order, 1u);
        const long long cnt = s.branch == DGC_BRANCH_RESAMPLE ? (long long)k : s.limit;   // final_count
        atomicAdd(&total, (unsigned long long)cnt);
        st->epoch = s.epoch + 1;
        // what the next K1 must zero (first-k branches of a deferring engine only)
        st->def_mode = (defer && s.branch != DGC_BRANCH_RESAMPLE && !tail && cnt > 0) ? 1 : 0;
        st->def_t = s.t_cur;
        st->def_limit = s.limit;
        st->def_mask_mmt = mask_mmt;
        if (info) {
            dgc_select_info& r = info[t];
            r.count = cnt;
            r.candidates = s.n_cur;
            r.threshold0 = s.t0;
            r.threshold = s.t_cur;
            r.branch = s.branch;
            r.recounts = s.recounts;
            r.overflow_segments = s.full_passes ? s.overflow : s.list_spills;
            r.full_passes = s.full_passes;
            r.tie_rule = s.tie_rule;
            r.window_keys = s.win_keys;
            r.k5_status = (int32_t)k5;
            r.list_threshold = used;   // (this call's; spec[0] is updated below)
        }
        if (spec) {
            // spec[0]: next call's list threshold = m x t x growth, growth = 2 - spec[1] / t
            //   (linear extrapolation from the previous final threshold spec[1]) clamped to
            //   [1, 1.5]; spec[1] := t. The ratio t / spec[1] overshoots while the growth
            //   decelerates (the accumulating velocity's threshold grows ~linearly). The
            //   margin m adapts: after a call whose threshold landed at or above its list
            //   threshold (a hit), m = 1.05 x that call's list/final ratio, within [margin,
            //   spec[4]] — the lists shrink towards the selection while the threshold moves
            //   predictably (at 1B on the bench's dynamics 4 % of the elements at 0.8 vs
            //   0.7 % at 0.95; ceiling 0.985: flat-1B's step 0.204 -> 0.179 ms past K1, same
            //   box); a miss (the threshold fell below it: a full select pass ran) resets m
            //   to margin and lowers the ceiling spec[4]. A prediction from the SAMPLED threshold series, with
            //   the lower of the last two final/sampled ratios (lists that hold a lowered
            //   threshold's candidates), was measured and dropped: on ResNet-50 its longer
            //   lists cost the list counts and the lowering 23 + 14 + 25 us where these take
            //   14 + 5 + 5, and the full passes stayed (same box, 0.372 vs 0.337 ms/step).
            const float tc = s.t_cur;
            const bool finite = tc == tc && tc > 0.f && tc < __builtin_huge_valf();
            const float gr = fminf(fmaxf(2.f - prev / tc, 1.f), 1.5f);   // first call: 2 - inf -> 1
            // the ceiling learns how closely t follows its prediction: it climbs while the
            // lists hold t (a hit) and steps down after a miss — a threshold that jitters
            // keeps its lists wider, a steady one (the bench's) narrows them to ~1.5 %
            const float c0 = spec[4] < __builtin_huge_valf() ? spec[4] : fmaxf(margin, kSpecCeil0);
            const bool tried = used < __builtin_huge_valf() && tc > 0.f;
            const bool hit = tried && tc >= used;
            const float mcap = !tried ? c0
                                : hit ? fminf(c0 + kSpecCeilUp, fmaxf(margin, kSpecMarginMax))
                                      : fmaxf(c0 - kSpecCeilDown, margin);
            float m = margin;
            if (hit) m = fminf(fmaxf(1.05f * (used / tc), margin), mcap);
            spec[4] = mcap;
            spec[0] = finite ? tc * m * gr : __builtin_huge_valf();
            spec[1] = finite ? tc : __builtin_huge_valf();
            // spec[2]: next call's sample-window threshold = mw x t0 x growth0, growth0 =
            //   2 - spec[3] / t0 clamped to [1, 1.5] (the sampled threshold's own linear
            //   extrapolation), spec[3] := t0. The window must hold >= ks samples and, for
            //   the one-workgroup select (rs_window_wg), <= kWinMax: mw = 0.97 after a window
            //   of that size, 0.985 after a larger one, 0.9 after one that missed (fewer than
            //   ks samples above it: this call's threshold came from the passes over every
            //   sample). The list threshold's margin (~0.95) put 8 ks samples in the window
            //   at 1B, past one workgroup's registers.
            const float t0 = s.t0;
            const bool f0 = t0 == t0 && t0 > 0.f && t0 < __builtin_huge_valf();
            const float g0 = fminf(fmaxf(2.f - spec[3] / t0, 1.f), 1.5f);
            const float mw = wc > (uint32_t)kWinMax ? 0.985f : (s.win_keys > 0 ? 0.97f : 0.9f);
            spec[2] = f0 ? t0 * mw * g0 : __builtin_huge_valf();
            spec[3] = f0 ? t0 : __builtin_huge_valf();
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && count_out) *count_out = (int64_t)total;
    if (threadIdx.x == 0 && f.order_out) *f.order_out = topk_order ? 0 : (int64_t)DGC_ORDER_ASCENDING;
    if (threadIdx.x == 0 && broken && f.sink)
        __hip_atomic_store(f.sink, (int32_t)broken, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ void k_sel_finish(SelWS w, FinishArgs f) { sel_finish_body(w, f); }

// K5 emit: output slot q <- candidate queue[q] (the topk's order), with values,
// wire casts and the masking of DGCSGDMemory.update.
__global__ void __launch_bounds__(kBlock) k_emit_queue(const float* __restrict__ vec_flat, SelWS w, EmitOut o) {
    const int t = task(w, BT_QUEUE, blockIdx.x);
    const SelState* st = w.st + t;
    if (!(st->branch == DGC_BRANCH_RESAMPLE && st->rs_nth == 1)) return;
    const TDesc d = w.td[t];   // by value: stores below cannot alias it
    __shared__ long long obase_s;
    if (threadIdx.x < kWave) {
        const long long b = out_base(w, t);
        if (threadIdx.x == 0) obase_s = b;
    }
    __syncthreads();
    const int64_t q = ((int64_t)blockIdx.x - w.bt[BT_QUEUE][t]) * kQueuePerBlock + threadIdx.x;
    if (q >= d.k) return;
    const uint32_t j = (uint32_t)w.queue[d.cand_off + q];
    emit_one(o, d, obase_s + q, w.cand_idx[d.cand_off + j], w.cand_val[d.cand_off + j]);
}
}  // namespace dgc
