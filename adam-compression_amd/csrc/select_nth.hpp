// Selection, K5: k_nth_select — the nth_element replay (introselect.hpp) with its
// multi-workgroup global phase, the partial_sort replay (select_heap.hpp), the queue
// emit and, by its last workgroup, the call's finish. Relies on select_emit.hpp
// (EmitOut, emit_one, FinishArgs, sel_finish_body) and select_heap.hpp.
#pragma once
#include "select_heap.hpp"

namespace dgc {
// Grid T x G: workgroup (t, 0) replays tensor t. global_here (G > 1): the tensor's G
// workgroups (t, 0..G-1) first run K5's global phase (nth_global_multi, its stopper
// bytes in the replay's LDS area, which is free until the phase ends); the replay goes
// on from the state the phase left, and workgroups (t, b > 0) leave after it, or stay
// to emit the queue (queue_here, below).
// The last of the T workgroups (t, 0) to finish (f.on) then runs the finish of the whole
// call (T arrivals on one ticket; nothing it writes is read by k_emit_queue).
//
// A global phase that BROKE (a barrier timed out after the consensus voted GO: its
// partitions of the queue are not reliable) is recovered here, in the same call: the
// queue is rebuilt from the gather's candidate keys — entry j = (key_j << 32 | j), as
// the gather wrote it — and the whole nth_element replayed on this workgroup from
// [0, n), exact (k5_status DGC_K5_FALLBACK | DGC_K5_RECOVERED). force_broken (parity
// tests, DGC_K5_FORCE_BROKEN=1): every replayed tensor takes that path, its queue first
// overwritten with garbage.
// queue_here (k > kQueueFold somewhere, and G > 1 workgroups per tensor): the extra
// workgroups (t, 1..G-1) of a replayed tensor wait for its replay (NthG::replayed) and
// write its k entries in the replayed order, a share each — k_emit_queue, a ~5 us
// launch that is a no-op in every step without a replay (flat-1B, VGG-16-BN), is not
// launched. The wait is bounded (~seconds; workgroup (t, 0) never waits on them): past
// it the payload is incomplete and the call reports DGC_K5_BROKEN through the sink.
__global__ void __launch_bounds__(kNthThreads) k_nth_select(const float* __restrict__ vec_flat, SelWS w,
                                                            EmitOut o, FinishArgs f, int force_broken,
                                                            int emit_here, int global_here, uint32_t G,
                                                            int64_t min_run, uint32_t G_expected, int queue_here,
                                                            int rebuild_queue) {
    const int t = blockIdx.x;
    const uint32_t b = blockIdx.y;
    const SelState* st = w.st + t;
    __shared__ __align__(16) uint64_t smem[kK5SmemBytes / 8];
    static_assert(kK5SmemBytes >= (size_t)kNthGMk, "the global phase's stopper bytes fit the replay's LDS");
    if (global_here && st->branch == DGC_BRANCH_RESAMPLE && st->rs_nth == 1) {   // uniform per tensor
        const TDesc d = w.td[t];
        uint32_t* gl = w.gpos + d.gpos_off;
        uint32_t* gr = gl + d.cand_cap / 2 + 1;
        nth_global_multi(w.queue + d.cand_off, st->n_cur, d.k - 1, gl, gr, w.nthg + t, b, G, min_run, G_expected,
                         reinterpret_cast<DGC_LDS uint8_t*>(lds(smem)));
        __syncthreads();   // (smem is the replay's from here)
    }
    if (b > 0) {
        if (queue_here && st->branch == DGC_BRANCH_RESAMPLE && st->rs_nth == 1) {   // uniform per tensor
            NthG* g = w.nthg + t;
            __shared__ int ready;
            __shared__ long long qbase_s;
            if (threadIdx.x == 0) {
                bool done = false;
                for (uint32_t spin = 0; spin < (1u << 26); ++spin) {
                    if (__hip_atomic_load(&g->replayed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                        done = true;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(2);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                if (!done) {
                    atomicOr(&g->status, (uint32_t)DGC_K5_BROKEN);
                    raise_flag(f.sink, (int32_t)DGC_K5_BROKEN);
                }
                ready = done;
            }
            __syncthreads();
            if (!ready) return;   // uniform
            if (threadIdx.x < kWave) {
                const long long ob = out_base(w, t);
                if (threadIdx.x == 0) qbase_s = ob;
            }
            __syncthreads();
            const TDesc d = w.td[t];
            const int64_t share = ceil_div(d.k, (int64_t)(G - 1));
            const int64_t q0 = (int64_t)(b - 1) * share, q1 = q0 + share < d.k ? q0 + share : d.k;
            for (int64_t q = q0 + threadIdx.x; q < q1; q += kNthThreads) {
                const uint32_t j = (uint32_t)w.queue[d.cand_off + q];
                emit_one(o, d, qbase_s + q, w.cand_idx[d.cand_off + j], w.cand_val[d.cand_off + j]);
            }
        }
        return;
    }
    K5_STAMP(7);
    if (st->branch == DGC_BRANCH_RESAMPLE && st->rs_nth == 2) {   // uniform per workgroup
        heap_select_wg(vec_flat, w, o, t, smem);
    } else if (st->branch == DGC_BRANCH_RESAMPLE && st->rs_nth == 1) {
        const TDesc d = w.td[t];   // by value: stores below cannot alias it
        DGC_GLB uint32_t* gl = glb(w.gpos + d.gpos_off);
        DGC_GLB uint32_t* gr = gl + d.cand_cap / 2 + 1;
        DGC_LDS uint64_t* lq = lds(smem);
        DGC_LDS uint32_t* llp = reinterpret_cast<DGC_LDS uint32_t*>(lq + kNthLds);
        DGC_LDS uint32_t* lrp = llp + kNthPairLds;
        DGC_LDS uint8_t* lmk = reinterpret_cast<DGC_LDS uint8_t*>(lrp + kNthPairLds);
        NthG* g = w.nthg + t;
        DGC_GLB uint64_t* q = glb(w.queue + d.cand_off);
        const int64_t nc = st->n_cur;
        __shared__ int recover;
        if (threadIdx.x == 0)
            recover = force_broken ||
                      (global_here && (__hip_atomic_load(&g->status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) &
                                       (uint32_t)DGC_K5_BROKEN));
        __syncthreads();
        if (recover) {
            // a GO phase's workgroups may still be on their way out of a timed-out barrier:
            // none touches the queue once it has counted itself
            if (global_here && threadIdx.x == 0 &&
                __hip_atomic_load(&g->decide, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kNthGGo)
                while (__hip_atomic_load(&g->exited, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < G)
                    __builtin_amdgcn_s_sleep(2);
            __syncthreads();
            if (force_broken)
                for (int64_t j = threadIdx.x; j < nc; j += kNthThreads) q[j] = ~(uint64_t)j;
            __syncthreads();
            const DGC_GLB uint32_t* ck = glb(w.cand_key + d.cand_off);
            for (int64_t j = threadIdx.x; j < nc; j += kNthThreads) q[j] = ((uint64_t)ck[j] << 32) | (uint64_t)j;
            __syncthreads();
            if (threadIdx.x == 0)
                g->status = (g->status & ~(uint32_t)DGC_K5_BROKEN) | (uint32_t)(DGC_K5_FALLBACK | DGC_K5_RECOVERED);
        } else if (rebuild_queue) {   // the gather wrote no queue (an index-order engine, no global phase)
            const DGC_GLB uint32_t* ck = glb(w.cand_key + d.cand_off);
            for (int64_t j = threadIdx.x; j < nc; j += kNthThreads) q[j] = ((uint64_t)ck[j] << 32) | (uint64_t)j;
            __syncthreads();
        }
        nth_element_wg(q, nc, d.k - 1, gl, gr, lq, llp, lrp, lmk, global_here && !recover ? g : nullptr);
        if (queue_here) {   // the replayed order is in the queue: the extra workgroups emit it
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (threadIdx.x == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                __hip_atomic_store(&g->replayed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else if (emit_here) {
            // the replayed order out by this workgroup (k <= kQueueFold for every tensor of
            // the call: no k_emit_queue launch); the payload position is known, every
            // tensor's branch and count being final before K5 runs
            __shared__ long long obase_s;
            __syncthreads();
            if (threadIdx.x < kWave) {
                const long long b = out_base(w, t);
                if (threadIdx.x == 0) obase_s = b;
            }
            __syncthreads();
            const long long ob = obase_s;
            for (int64_t q0 = threadIdx.x; q0 < d.k; q0 += kNthThreads) {
                const uint32_t j = (uint32_t)q[q0];
                emit_one(o, d, ob + q0, w.cand_idx[d.cand_off + j], w.cand_val[d.cand_off + j]);
            }
        }
    }
    const bool idle = !(st->branch == DGC_BRANCH_RESAMPLE && (st->rs_nth == 1 || st->rs_nth == 2));
    if (idle) K5_STAMP(0);   // (profiling build: slots 0-2 are free when the replay did not run)
    if (f.on && last_block_arrival(w.fin_ticket, gridDim.x)) {
        if (idle) K5_STAMP(1);
        sel_finish_body(w, f);
        if (idle) K5_STAMP(2);
    }
    K5_STAMP(6);
}
}  // namespace dgc
