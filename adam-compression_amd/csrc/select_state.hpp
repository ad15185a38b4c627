// Selection, per-tensor state machine: sel_init_tensor (a call's reset; run by K3's
// kernels and k_sel_init), block_scan_array, and decide_tensor — the reference's
// adaptation step, taken by the last workgroup of every count pass (select_count.hpp,
// select_emit.hpp). Relies on select_types.hpp.
#pragma once
#include "select_types.hpp"

namespace dgc {
// Reset tensor t's selection state for this call, by the whole calling workgroup (any
// size): the workgroup that just produced its sampled threshold (k_rs_small_multi, or
// the last workgroup of k_rs_passes' final pass — no launch of its own), or
// k_sel_init for a pure selection (dgc_select, the threshold given).
__device__ void sel_init_tensor(const SelWS& w, int t, int keep_lists) {
    const TDesc d = w.td[t];   // by value: stores below cannot alias it
    SelState* st = w.st + t;
    __shared__ uint32_t setg_broken;
    if (threadIdx.x == 0) {   // K5's multi-workgroup barrier and consensus start from zero
        w.nthg[t].bar_count = 0;
        w.nthg[t].bar_gen = 0;
        w.nthg[t].arrive = 0;
        w.nthg[t].decide = 0;
        w.nthg[t].status = 0;
        w.nthg[t].exited = 0;
        w.nthg[t].replayed = 0;
        SetG& sg = w.setg[t];
        setg_broken = sg.broken;
        sg.arrive = sg.decide = sg.bar_count = sg.bar_gen = sg.broken = sg.gathered = 0;
        sg.mn = 0xFFFFFFFFu;
        sg.mx = 0;
        if (t == 0) *w.fin_ticket = 0;
    }
    // k_chain_one's words (k_rs_passes', past kChainOneWords, are zero at rest); one store
    // per thread (every caller runs >= kBlock threads): a strided loop here gave
    // k_rs_small_multi a 320 B/lane scratch frame and doubled its time (15 -> 29 us)
    static_assert(kChainOneWords <= kBlock, "sel_init_tensor: one chain word per thread");
    if (t == 0 && threadIdx.x < kChainOneWords) w.chain[threadIdx.x] = 0;
    __shared__ uint32_t spills;
    if (threadIdx.x == 0) spills = 0;
    __syncthreads();   // the caller's threshold (thr[t]) is written
    if (setg_broken) {
        // a barrier of this tensor's last K5s timed out: its workgroups may have run
        // different numbers of passes, leaving merged-histogram bins they did not re-zero
        // (or re-zeroed before a late add) — restore "zero at rest" for the whole table
        SetG& sg = w.setg[t];
        for (int q = threadIdx.x; q < kSetBins0; q += blockDim.x) sg.hist0[q] = 0;
        for (int q = threadIdx.x; q < kSetBins1; q += blockDim.x) sg.hist1[q] = 0;
    }
    // every load of the reset in flight at once — the epoch, both spill slots, the
    // threshold, the window count: as three dependent round trips they were ~3 us of K3
    const int ep = st->epoch;
    uint32_t sp0 = 0, sp1 = 0;
    if (threadIdx.x < kSpillShards) {
        sp0 = st->spill[0][threadIdx.x];
        sp1 = st->spill[1][threadIdx.x];
    }
    float t0 = 0.f;
    uint32_t win_n = 0;
    if (threadIdx.x == 0) {
        t0 = w.thr[t];
        win_n = w.rs[t].win_n;
    }
    for (int64_t i = threadIdx.x; i < d.ngrp; i += blockDim.x) {
        w.grp_cnt[d.grp0 + i] = 0;
        w.grp_lb[d.grp0 + i] = 0;
    }
    const int e = ep & 1;
    if (threadIdx.x < kSpillShards) {
        const uint32_t v = e ? sp1 : sp0;
        if (v) atomicAdd(&spills, v);
        st->spill[e ^ 1][threadIdx.x] = 0;   // slot of the next call's K1
    }
    if (threadIdx.x == 0) {
        st->win_cnt[e ^ 1] = 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        st->win_keys = (d.win_cap > 0 && !d.tail) ? (int32_t)win_n : 0;
        st->t0 = t0;
        st->t_cur = t0;
        st->list_spills = keep_lists ? (int32_t)spills : 0;
        // no K1 lists, or too many overflowed lists to be worth serving: one full pass
        if (!keep_lists || (int64_t)spills * kSpillDiv > d.nseg) st->t_list = __builtin_huge_valf();
        st->branch = -1;
        st->n_cur = st->limit = 0;
        st->iter = st->recounts = 0;
        st->active = 1;
        st->overflow = 0;
        st->done = 0;
        st->lower_pending = 0;
        st->full_passes = 0;
        st->rs_nth = 0;
        st->tie_rule = DGC_TIES_NONE;
        for (int i = 0; i < 4; ++i) st->tickets[i] = 0;
        for (int i = 0; i < 9; ++i) st->tk8[i] = 0;
        for (int i = 0; i <= kMaxLower; ++i) st->lower_cnt[i] = 0;
        st->ce_ticket = 0;
        st->ce_fail = 0;
        st->spec_emitted = 0;
    }
}

// Chunked exclusive scan of a[0..m) into out[] by one workgroup; returns the total.
// a[] holds totals accumulated by device atomics: read with agent-scope loads, in
// chunks of kScanReg kept in registers so a chunk's loads are in flight together (a
// loop of dependent loads pays an L2 round trip each); a thread's run of <= kScanReg
// entries is loaded once.
constexpr int kScanReg = 8;
__device__ uint64_t block_scan_array(const unsigned long long* a, long long* out, int64_t m, uint64_t* lds16) {
    const int64_t per = ceil_div(m, (int64_t)blockDim.x);
    const int64_t b = threadIdx.x * per, e = b + per < m ? b + per : m;
    uint64_t v[kScanReg];
    uint64_t local = 0;
    for (int64_t i0 = b; i0 < e; i0 += kScanReg) {
#pragma unroll
        for (int u = 0; u < kScanReg; ++u) v[u] = i0 + u < e ? load_count(&a[i0 + u]) : 0;
#pragma unroll
        for (int u = 0; u < kScanReg; ++u) local += v[u];
    }
    uint64_t total;
    uint64_t run = block_exclusive_scan(local, lds16, &total);
    for (int64_t i0 = b; i0 < e; i0 += kScanReg) {
        if (per > kScanReg) {
#pragma unroll
            for (int u = 0; u < kScanReg; ++u) v[u] = i0 + u < e ? load_count(&a[i0 + u]) : 0;
        }
#pragma unroll
        for (int u = 0; u < kScanReg; ++u)
            if (i0 + u < e) {
                out[i0 + u] = (long long)run;
                run += v[u];
            }
    }
    return total;
}

// One step of the reference's adaptation loop (dgc/compression.py:128-149) on the
// count of the pass that just ran, for tensor t, by the whole calling workgroup (any
// size): the workgroup of the count pass that arrived last for the tensor (no launch
// of its own). With resample (the default) the loop can only lower the threshold until
// the count reaches lower*k, so the first "lower" step hands over to ONE
// multi-threshold pass (k_lower_counts) instead of recounting one threshold per pass;
// without resample the threshold may also rise, and each step is a recount (count
// pass + decide), like the reference. The group totals are other workgroups' device
// atomics of this launch: read with agent-scope loads (last_block_arrival).
__device__ void decide_tensor(const SelWS& w, const SelCfg& p, int t, int spec = 0) {
    SelState* st = w.st + t;
    const TDesc d = w.td[t];   // by value: stores below cannot alias it
    __shared__ uint64_t lds16[16];
    __shared__ int finished;
    uint64_t local = 0;
    // 8 loads in flight per thread: a 7B tensor has ~6700 groups, 26 per thread of a
    // 256-thread workgroup — one agent-scope round trip each when issued one by one
    const int64_t bd = blockDim.x;
    for (int64_t i0 = threadIdx.x; i0 < d.ngrp; i0 += 8 * bd) {
        uint64_t v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = i0 + u * bd < d.ngrp ? load_count(&w.grp_cnt[d.grp0 + i0 + u * bd]) : 0;
#pragma unroll
        for (int u = 0; u < 8; ++u) local += v[u];
    }
    uint64_t n;
    block_exclusive_scan(local, lds16, &n);
    if (threadIdx.x == 0) {
        if (st->t_cur < st->t_list) {   // a full select pass just re-listed at t_cur
            st->t_list = st->t_cur;
            st->full_passes += 1;
        }
        const long long cnt = (long long)n, k = d.k;
        const bool adapt = d.n > d.S;
        st->n_cur = cnt;
        int done = 1;
        if (!adapt) {
            st->branch = DGC_BRANCH_DIRECT;
            st->limit = cnt < k ? cnt : k;
        } else if (st->iter >= p.max_iters) {
            st->branch = DGC_BRANCH_EXHAUSTED;
            st->limit = cnt < k ? cnt : k;
        } else if (cnt > k) {
            if (cnt > d.upper_count) {
                if (p.resample) {
                    st->branch = DGC_BRANCH_RESAMPLE;
                    // torch's CPU topk: nth_element while k * 64 > candidates (K5), else
                    // partial_sort (K5b) — both replayed exactly
                    st->rs_nth = (cnt < 64 * k && cnt <= d.cand_cap) ? 1 : 2;
                    st->tie_rule = DGC_TIES_EXACT;
                } else {
                    st->t_cur = thr_mul(st->t_cur, p.upper, p.tdtype);
                    done = 0;
                }
            } else {
                st->branch = DGC_BRANCH_TRUNC;
                st->limit = k;
            }
        } else if (cnt < d.lower_count) {
            if (p.resample && st->iter == 0 && p.max_iters <= kMaxLower) {
                st->lower_pending = 1;   // k_lower_counts finds the final threshold in one pass
                done = 2;
            } else {
                st->t_cur = thr_mul(st->t_cur, p.lower, p.tdtype);
                done = 0;
            }
        } else {
            st->branch = DGC_BRANCH_OK;
            st->limit = cnt;
        }
        if (done == 0) {
            st->iter += 1;
            st->recounts += 1;
            st->overflow = 0;
        } else if (done == 1) {
            st->active = 0;
            st->done = 1;
            // a first-k branch after k_count_emit: its speculative payload is the emit
            if (spec && st->branch != DGC_BRANCH_RESAMPLE && !st->ce_fail) st->spec_emitted = 1;
        } else {
            st->active = 0;
        }
        finished = done;
    }
    __syncthreads();
    if (finished == 1) block_scan_array(w.grp_cnt + d.grp0, w.grp_off + d.grp0, d.ngrp, lds16);
    __syncthreads();
    if (finished != 1)
        for (int64_t i = threadIdx.x; i < d.ngrp; i += blockDim.x) w.grp_cnt[d.grp0 + i] = 0;
}

__global__ void __launch_bounds__(kScanThreads) k_sel_init(SelWS w, int keep_lists) {
    sel_init_tensor(w, blockIdx.x, keep_lists);
}
}  // namespace dgc
