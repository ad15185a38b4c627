// K4: selection — the `importance >= threshold` mask, `nonzero()`, the adaptation
// loop, resample, truncation, value gather, momentum masking and wire packing —
// plus the listing K1 of the fused compress and the K3 thresholds, for ONE tensor or
// for a BATCH of T tensors in the same launches.
//
// Reference: DGCCompressor._sparsify (dgc/compression.py:109-153),
// DGCSGDMemory.update (dgc/memory.py:72-77), compress's casts (dgc/compression.py:168-171),
// compress's call order (dgc/compression.py:155-172); the batch serves every
// compressed tensor of a step, which the reference handles one hook at a time
// (dgc/horovod/optimizer.py:116-155).
//
// Layout. A tensor's elements are cut into SEGMENTS of 1024; 1024 segments form a
// GROUP (the scan granule and one emit workgroup). In a batch the tensors sit at
// segment-aligned offsets of flat grad/mmt/vec buffers; segments and groups are
// numbered globally, and every launch maps each workgroup to ONE tensor through a
// prefix table of per-tensor block counts (task_of_block), so per-tensor state,
// per-tensor tickets and group atomics never mix tensors. Every segment owns a
// candidate list of kCap = 64 slots (u16 offset + fp32 value, ascending) and two
// exact counts: seg_lcnt at the LIST threshold t_list (complete iff <= kCap; a
// spilled segment is re-read from vec when needed) and seg_cnt at the current
// threshold t_cur >= t_list.
//
// Speculative listing. K1 lists candidates at t_list = margin x (the previous call's
// final threshold), per tensor. When the sampled threshold comes out >= t_list — the
// steady state — every count and selection is served from the lists and the separate
// 4 B/elem re-read of vec disappears; otherwise a full select pass at t_cur re-lists.
// Results are identical either way: a list at t_list holds EVERY element >= t_list.
//
//   count pass   t_cur >= t_list: one thread per segment counts its list entries
//                (spilled segments: one wave re-reads 1024 elements); else the full
//                select pass (16 non-temporal float4 loads in flight per lane).
//   decide       (1 workgroup per tensor): the reference's loop step (ok / trunc /
//                resample / lower / raise / exhausted) + scan of the group totals.
//                resample=True: the first "lower" hands over to ONE multi-threshold
//                pass; resample=False: a recount per step.
//   resample     torch's CPU topk replayed exactly: nth_element path (candidates <
//                64 k): the candidates are gathered in index order and the introselect
//                replayed (K5, introselect.hpp); partial_sort path: heap select +
//                sort_heap over vec (K5b, heap_select_wg).
//   emit         (1 workgroup per group): positions (after the tensors before it in
//                the batch), fp32/fp16 values, int64/int32 indices, masking writes.
//
// Everything is stream-ordered; in DGC_SYNC_DEVICE mode kernels that turn out to
// be unneeded early-exit on a device flag, so no host synchronisation happens.
//
// The stages live in headers, all compiled into this one translation unit (so inlining and
// the DGC_K5_PROF device globals stay as they were), included below in definition order;
// this file keeps the host driver, the one-tensor and batch plumbing and the C ABI.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>

#include "dispatch.hpp"             // with_*: run-time dtype / flag -> template argument
#include "payload.hpp"              // payload layout, shared argument checks
#include "select_types.hpp"        // constants, list slots, TDesc / SelState / SetG / SelCfg / SelWS
#include "select_layout.hpp"       // host layout, workspace carve, k_put_one / k_put_starts
#include "select_tiles.hpp"        // tile loads, list append, task(), deferred masking
#include "select_k1.hpp"           // K1 with lists over fp32 state (an fp32 or, the flat bucket, a 16-bit gradient)
#include "select_k1_16.hpp"        // K1 with lists over 16-bit state (the flat bucket)
#include "select_state.hpp"        // sel_init_tensor, decide_tensor
#include "select_thresholds.hpp"   // K3
#include "select_count.hpp"        // list count, select pass, lowering
#include "select_emit.hpp"         // k_emit, k_chain_one, wide emit, count-emit, finish, k_emit_queue
#include "select_heap.hpp"         // K5b heap replay
#include "select_set.hpp"          // K5s cooperative set
#include "select_nth.hpp"          // K5 k_nth_select

namespace dgc {

__global__ void k_spec_reset(float* spec, int32_t T) {
    for (int i = threadIdx.x; i < kSpecWords * T; i += blockDim.x) spec[i] = __builtin_huge_valf();
}

// ------------------------------------------------------------------ host driver
// The resample replays pack what they move into 64-bit entries: K5's queue holds
// (key << 32 | candidate position), K5b's heap (key31 << 33 | element index, or a slot
// of the k heap entries with the index beside it from N = 2^33 on). A tensor whose
// candidates do not fit K5's width is refused up front — torch's topk takes any n
// (dgc/compression.py:124-137), and a truncated position would be a wrong payload, not
// an error. (k < 2^32 follows: the candidate capacity min(64k - 1, n) is >= k.)
static int check_replay_width(int64_t n, int64_t k, const char* who) {
    if (nth_cand_cap(n, k) > (int64_t)0xFFFFFFFFLL)
        DGC_FAIL(DGC_ERR_OVERFLOW,
                 "%s: the resample replay addresses at most 2^32 - 1 candidates; numel %lld with num_selects %lld "
                 "can have %lld (use resample=False or a smaller tensor)",
                 who, (long long)n, (long long)k, (long long)nth_cand_cap(n, k));
    return DGC_OK;
}

static int validate_select(const dgc_select_params* p, void* values, void* indices) {
    if (!p) DGC_FAIL(DGC_ERR_INVALID, "dgc_select: null params");
    if (p->numel < 1 || p->num_selects < 1 || p->num_selects > p->numel)
        DGC_FAIL(DGC_ERR_INVALID, "dgc_select: need 1 <= num_selects <= numel (got %lld, %lld)",
                 (long long)p->num_selects, (long long)p->numel);
    if (p->num_samples < 1 || p->num_samples > p->numel)
        DGC_FAIL(DGC_ERR_INVALID, "dgc_select: bad num_samples");
    if (p->max_iters < 0) DGC_FAIL(DGC_ERR_INVALID, "dgc_select: max_iters < 0");
    if (!wire_ok(p->vdtype, true)) DGC_FAIL(DGC_ERR_DTYPE, "dgc_select: value dtype");
    if (!float_dtype_ok(p->thr_dtype)) DGC_FAIL(DGC_ERR_DTYPE, "dgc_select: threshold dtype");
    if (!index_ok(p->idtype)) DGC_FAIL(DGC_ERR_DTYPE, "dgc_select: index dtype");
    if (p->idtype == DGC_I32 && p->numel > 2147483647LL)
        DGC_FAIL(DGC_ERR_OVERFLOW, "dgc_select: int32 indices cannot address %lld elements",
                 (long long)p->numel);
    if (p->resample) DGC_TRY(check_replay_width(p->numel, p->num_selects, "dgc_select"));
    if (!values || !indices) DGC_FAIL(DGC_ERR_INVALID, "dgc_select: null outputs");
    return DGC_OK;
}

static SelCfg cfg_of(const dgc_select_params& p) {
    return SelCfg{p.upper, p.lower,       p.max_iters,     p.resample,  p.masking,
                  p.vdtype, p.idtype,     p.update_memory, p.thr_dtype, p.resample_order == 1 ? 1 : 0};
}

// The library's only environment switches, all three for the parity
// tests, which reach at small sizes the paths that only large tensors take. Read on every
// call: the tests set them in-process.
struct TestHooks {
    int emit_shape;      // DGC_EMIT_SHAPE=quarter|wide: 0 unset, 1 wide, -1 anything else (k_emit)
    bool k5_wg;          // DGC_K5_GLOBAL=wg: K5's global phase on one workgroup
    bool k5_multi;       // DGC_K5_GLOBAL=multi|abort: on several, whatever the candidate counts
    bool k5_abort;       // DGC_K5_GLOBAL=abort: ... one workgroup short, so the consensus times out
    int force_broken;    // DGC_K5_FORCE_BROKEN: every replayed tensor recovers a broken global phase
};

static TestHooks test_hooks() {
    const char* shape = std::getenv("DGC_EMIT_SHAPE");
    const char* k5 = std::getenv("DGC_K5_GLOBAL");
    TestHooks h{};
    h.emit_shape = !shape ? 0 : std::strcmp(shape, "wide") == 0 ? 1 : -1;
    h.k5_wg = k5 && std::strcmp(k5, "wg") == 0;
    h.k5_abort = k5 && std::strcmp(k5, "abort") == 0;
    h.k5_multi = h.k5_abort || (k5 && std::strcmp(k5, "multi") == 0);
    h.force_broken = std::getenv("DGC_K5_FORCE_BROKEN") ? 1 : 0;
    return h;
}

// k_emit for many groups (flat buckets), k_emit_wide for few (model gradient sets).
static bool emit_is_wide(const Layout& L, const TestHooks& hooks) {
    return hooks.emit_shape ? hooks.emit_shape > 0 : L.ngrp < 256;
}

static int launch_emit(const Layout& L, const float* vec, const SelWS& w, const EmitOut& o, const TestHooks& hooks,
                       hipStream_t s) {
    if (emit_is_wide(L, hooks))
        hipLaunchKernelGGL(k_emit_wide_t<false>, dim3((unsigned)L.grid[BT_GRP]), dim3(kGroupSegs), 0, s, vec, w, o, o,
                           (int32_t)L.grid[BT_GRP]);
    else
        hipLaunchKernelGGL(k_emit, dim3((unsigned)L.grid[BT_GRP]), dim3(kEmitSegs), 0, s, vec, w, o);
    DGC_LAUNCHED();
    return DGC_OK;
}

// Workgroups per tensor for K5's global phase (k_nth_select's extra workgroups): half
// the CUs shared among the T tensors, at most kNthGMax. They wait for each other, so all
// of them must be resident at once: <= CUs / 2 workgroups of 8 waves (one fits a CU with
// k_nth_select's ~150 KB of LDS) guarantee that with this stream's earlier kernels done.
// (hipLaunchCooperativeKernel checks the same but cost ~29 us per launch on MI355X: more
// than the phase saves below ~200k candidates.)
// <= 1 keeps the whole replay on one workgroup per tensor; so does a call whose tensors
// all have candidate capacities <= kNthGMinCand, and so does a tensor with <=
// kNthGMinCand candidates (decided on the device: below ~100k the three cross-XCD
// barriers per step cost as much as the spread saves), and the
// parity tests' DGC_K5_GLOBAL=wg; their DGC_K5_GLOBAL=multi skips both gates.
constexpr int64_t kNthGMinCand = 98304;    // launch for capacities above, run for candidate counts above

static uint32_t nth_global_groups(int32_t T, int64_t max_cand, const TestHooks& hooks) {
    static int per_dev = -1;
    if (per_dev < 0) {
        int dev = 0, cus = 0, per_cu = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(k_nth_select),
                                                         kNthThreads, 0) != hipSuccess)
            per_dev = 0;
        else
            per_dev = per_cu >= 1 ? cus / 2 : 0;

    }
    if (hooks.k5_wg) return 0;
    const bool multi = hooks.k5_multi;
    if (max_cand <= kNthLds || (max_cand <= kNthGMinCand && !multi)) return 0;
    // measured: 16 workgroups per tensor for every tensor of a batch
    // from 40k candidates made ResNet-50 0.358 -> 0.373 ms (864 workgroups launched per
    // step, and at 45-57k candidates the spread phase is no faster than one workgroup:
    // 0.141-0.144 ms either way); it pays from ~100k (500k: 0.945 -> 0.371 ms)
    // fewer than 4 per tensor (a batch of many tensors: ResNet-50's 54) spread too little
    // to pay the barriers, and the launch alone is ~5.7 us per step (rocprofv3)
    const int64_t g = T > 0 ? per_dev / T : 0;
    if (g < 4 && !multi) return 0;
    return (uint32_t)std::min<int64_t>(g, kNthGMax);
}

// ---- the count passes of one selection call. A pass runs at t_cur: the list count where
// t_cur >= t_list, else the full select pass (both gated per tensor on the device); each
// count kernel's last workgroup per tensor takes the adaptation step. A kernel with an
// ALIGNED form is launched as `c.al ? k<true> : k<false>`.
struct SelCall {
    const float* vec;
    bool al;   // vec is 16-byte aligned (float4 loads)
    const SelWS& w;
    const SelCfg& p;
    const Layout& L;
    hipStream_t s;
};

// the list count and the full pass in one launch, the count also writing the first-k payload
static int launch_count_emit_pass(const SelCall& c, const EmitOut& o, bool likely_lists) {
    const int which = likely_lists ? BT_CAP16 : BT_FULL;
    const unsigned grid = (unsigned)(c.L.grid[BT_CNT] + c.L.grid[which]);
    hipLaunchKernelGGL(c.al ? k_count_emit_pass<true> : k_count_emit_pass<false>, dim3(grid), dim3(kBlock), 0, c.s,
                       c.vec, c.w, c.p, o, which, (int)c.L.grid[BT_CNT]);
    DGC_LAUNCHED();
    return DGC_OK;
}

// the list count and the full pass in one launch. A batch's full pass takes two segments
// per wave, a single tensor's kSuper. Measured (tools/pass_prof.py, ResNet-50): four per
// wave keep a working workgroup ~9 us on its list appends after 3 us of loads, one per
// wave ~3 us but 6289 workgroups enter over 10.7 us (the working ones hold the slots);
// two: 6 us each, all entered within 3.9 us, the pass ends at 15 instead of 18 us —
// ResNet-50 0.2269 -> 0.2235 ms, VGG-16-BN 0.6275 -> 0.6264 (4 alternations; one per
// wave 0.2310 / 0.6282)
static int launch_count_pass(const SelCall& c, bool likely_lists) {
    const bool two = c.L.T > 1;
    const int which = two ? (likely_lists ? BT_CAP8 : BT_FULL8) : (likely_lists ? BT_CAP16 : BT_FULL);
    const unsigned grid = (unsigned)(c.L.grid[BT_CNT] + c.L.grid[which]);
    const auto k = two ? (c.al ? k_count_pass<true, 2> : k_count_pass<false, 2>)
                       : (c.al ? k_count_pass<true, kSuper> : k_count_pass<false, kSuper>);
    hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), 0, c.s, c.vec, c.w, which, c.p, (int)c.L.grid[BT_CNT]);
    DGC_LAUNCHED();
    return DGC_OK;
}

// the list count alone; emit: it also writes the first-k payload (k_count_emit)
static int launch_count_lists(const SelCall& c, const EmitOut* emit) {
    if (emit)
        hipLaunchKernelGGL(k_count_emit, dim3((unsigned)c.L.grid[BT_CNT]), dim3(kBlock), 0, c.s, c.vec, c.w, c.p,
                           *emit);
    else
        hipLaunchKernelGGL(k_count_lists, dim3((unsigned)c.L.grid[BT_CNT]), dim3(kBlock), 0, c.s, c.vec, c.w, c.p);
    DGC_LAUNCHED();
    return DGC_OK;
}

// the full select pass alone
static int launch_select_pass(const SelCall& c, bool likely_lists) {
    const int which = likely_lists ? BT_CAP16 : BT_FULL;
    hipLaunchKernelGGL(c.al ? k_select_pass<true> : k_select_pass<false>, dim3((unsigned)c.L.grid[which]),
                       dim3(kBlock), 0, c.s, c.vec, c.w, which, c.p);
    DGC_LAUNCHED();
    return DGC_OK;
}

// The multi-threshold lowering. One tensor (the per-tensor path; the flat bucket chains
// its lowering, k_chain_one): from the K1 lists first, then over vec if they do not
// reach. A batch goes to vec at once: on per-step gradients a lowered threshold (0.8 t0)
// sits below the lists almost always, and the list launch cost ResNet-50 6 us,
// VGG-16-BN 4 (same box, 3 alternations).
static int launch_lower(const SelCall& c) {
    if (c.L.T == 1) {
        hipLaunchKernelGGL(k_lower_lists, dim3((unsigned)c.L.grid[BT_SEG]), dim3(kBlock), 0, c.s, c.vec, c.w, c.p);
        DGC_LAUNCHED();
    }
    hipLaunchKernelGGL((c.al ? k_lower_counts<true, 1> : k_lower_counts<false, 1>),
                       dim3((unsigned)c.L.grid[BT_CAP4]), dim3(kBlock), 0, c.s, c.vec, c.w, c.p);
    DGC_LAUNCHED();
    return DGC_OK;
}

// The resample's nth_element path: gather the candidates, replay the introselect, emit
// in its order. The gather launch also emits every other tensor's payload (the final
// emit), and k_nth_select's last workgroup finishes the call (f).
static int launch_resample(const SelCall& c, const EmitOut& o, FinishArgs f, const TestHooks& hooks) {
    const Layout& L = c.L;
    const uint32_t G = nth_global_groups(L.T, L.max_cand, hooks);
    // An index-order engine whose replay runs on one workgroup (no global phase): the
    // gather writes no queue — the sets read the keys, and the rare tied set that falls
    // to the replay has k_nth_select rebuild its queue from them (one of the gather's
    // four stores per candidate)
    const bool no_queue = c.p.set_order && G <= 1;
    EmitOut g = o;   // the K5 gather (+ every other tensor's payload)
    g.queue = c.w.queue;
    g.cand = c.w.cand_idx;
    g.cval = c.w.cand_val;
    g.ckey = c.w.cand_key;
    g.no_queue = no_queue ? 1 : 0;
    // K5s: an untied resample set in index order (the rest: the replay); with the wide
    // emit, in its launch (k_emit_set)
    const bool sets = c.p.set_order && L.grid[BT_SET] > 0;
    if (sets && emit_is_wide(L, hooks)) {
        hipLaunchKernelGGL(k_emit_wide_t<true>, dim3((unsigned)(L.grid[BT_GRP] + L.grid[BT_SET])), dim3(kGroupSegs),
                           0, c.s, c.vec, c.w, g, o, (int32_t)L.grid[BT_GRP]);
        DGC_LAUNCHED();
    } else {
        DGC_TRY(launch_emit(L, c.vec, c.w, g, hooks, c.s));
        if (sets) {
            hipLaunchKernelGGL(k_resample_set, dim3((unsigned)L.grid[BT_SET]), dim3(kScanThreads), 0, c.s, c.vec, c.w,
                               o);
            DGC_LAUNCHED();
        }
    }
    // G > 1: the tensor's G workgroups run K5's global phase, then the extra ones emit
    // the queue unless the replay's own workgroup does (every k <= kQueueFold).
    // Parity tests: k5_multi runs the phase at any candidate count; k5_abort has the
    // kernel expect one workgroup more than launched, so the residency consensus times
    // out and the one-workgroup replay takes over.
    const bool global_here = G > 1;
    const bool emit_here = L.max_k <= kQueueFold;
    const bool queue_here = !emit_here && global_here;
    const int64_t min_run = hooks.k5_multi ? 0 : kNthGMinCand;
    const uint32_t G_expected = hooks.k5_abort ? G + 1 : G;
    f.on = 1;
    hipLaunchKernelGGL(k_nth_select, dim3((unsigned)L.T, global_here ? G : 1u), dim3(kNthThreads), 0, c.s, c.vec,
                       c.w, o, f, hooks.force_broken, emit_here ? 1 : 0, global_here ? 1 : 0, G,
                       min_run, G_expected, queue_here ? 1 : 0, no_queue ? 1 : 0);
    DGC_LAUNCHED();
    if (!emit_here && !queue_here) {
        hipLaunchKernelGGL(k_emit_queue, dim3((unsigned)L.grid[BT_QUEUE]), dim3(kBlock), 0, c.s, c.vec, c.w, o);
        DGC_LAUNCHED();
    }
    return DGC_OK;
}

// The selection of every tensor (its K1 lists kept or not), from k_sel_init to the
// payload: stream-ordered, and in DGC_SYNC_DEVICE mode with no host synchronisation.
static int select_core(float* vec, float* mmt, const SelCfg& p, const Layout& L, void* values, void* indices,
                       int64_t* count_out, dgc_select_info* info, const SelWS& w, int keep_lists, int sync_mode,
                       float margin, int32_t* sink, int64_t* order_out, hipStream_t s) {
    // keep_lists: a compress call, whose K3 kernels already reset every tensor's state
    // (sel_init_tensor) when they produced its threshold; a pure selection resets here
    if (!keep_lists) {
        hipLaunchKernelGGL(k_sel_init, dim3((unsigned)L.T), dim3(kScanThreads), 0, s, w, 0);
        DGC_LAUNCHED();
    }
    const TestHooks hooks = test_hooks();
    const SelCall c{vec, aligned16(vec), w, p, L, s};
    const bool device = sync_mode == DGC_SYNC_DEVICE;
    // resample=True with max_iters <= kMaxLower: one multi-threshold pass replaces the lowers
    const bool lower_fast = p.resample && p.max_iters <= kMaxLower;
    const EmitOut o{p.update_memory ? vec : nullptr, (p.update_memory && p.masking) ? mmt : nullptr, values, indices,
                    p.vdtype, p.idtype, nullptr, nullptr, (int32_t)(p.update_memory == 2)};
    const FinishArgs fin{count_out, info, margin, (int32_t)(p.update_memory == 2), (int32_t)(p.masking != 0), 0,
                         sink, 0u, order_out};
    // a pass where either the lists or vec may serve: in one launch when the decisions
    // stay on the device and the lowering is the one multi-threshold pass
    const bool merge_ok = lower_fast && device;
    auto pass_either = [&](bool likely_lists, const EmitOut* emit = nullptr) -> int {
        if (merge_ok) return emit ? launch_count_emit_pass(c, *emit, likely_lists) : launch_count_pass(c, likely_lists);
        DGC_TRY(launch_count_lists(c, emit));
        return launch_select_pass(c, likely_lists);
    };
    // the first list count of a one-tensor call also writes the first-k payload
    // (k_count_emit) when that emit would not mask and the payload starts at slot 0
    const bool fuse = keep_lists && L.T == 1 && !L.tail_any && device && (p.update_memory == 2 || p.update_memory == 0);
    DGC_TRY(keep_lists ? pass_either(true, fuse ? &o : nullptr) : launch_select_pass(c, false));
    bool resampled = false;   // launch_resample wrote every payload and finished the call
    if (!device) {
        // read the decisions back and launch only what they need
        std::vector<SelState> hs(L.T);
        for (;;) {
            DGC_HIP(hipMemcpyAsync(hs.data(), w.st, sizeof(SelState) * L.T, hipMemcpyDeviceToHost, s));
            DGC_HIP(hipStreamSynchronize(s));
            bool all_done = true, any_lower = false, any_full = false, any_list = false;
            for (const SelState& h : hs) {
                if (h.done) continue;
                all_done = false;
                if (h.lower_pending)
                    any_lower = true;
                else if (h.t_cur >= h.t_list)
                    any_list = true;
                else
                    any_full = true;
            }
            if (all_done) break;
            if (any_lower) {
                DGC_TRY(launch_lower(c));   // picks t_cur on the device: either pass may follow
                DGC_TRY(pass_either(false));
            } else {
                if (any_list) DGC_TRY(launch_count_lists(c, nullptr));
                if (any_full) DGC_TRY(launch_select_pass(c, false));
            }
        }
        for (const SelState& h : hs) resampled |= h.branch == DGC_BRANCH_RESAMPLE;
    } else if (L.adapt_any) {
        // every kernel below early-exits on a device flag when it is not needed
        if (L.T == 1 && keep_lists && lower_fast) {
            // one tensor: the lowering and the count at the lowered threshold in one
            // launch (k_chain_one), then its full pass
            const unsigned grid = (unsigned)std::min<int64_t>(
                kCapBlocks, std::max({L.grid[BT_SEG], L.grid[BT_CAP4], L.grid[BT_CNT]}));
            hipLaunchKernelGGL(c.al ? k_chain_one<true> : k_chain_one<false>, dim3(grid), dim3(kBlock), 0, s, vec, w,
                               p);
            DGC_LAUNCHED();
            DGC_TRY(launch_select_pass(c, true));
        } else if (lower_fast) {
            DGC_TRY(launch_lower(c));
            DGC_TRY(pass_either(true));
        } else {
            for (int i = 0; i < p.max_iters; ++i) DGC_TRY(pass_either(true));
        }
        resampled = p.resample != 0;
    }
    if (resampled) return launch_resample(c, o, fin, hooks);   // k_nth_select serves both paths (K5, K5b)
    DGC_TRY(launch_emit(L, vec, w, o, hooks, s));
    hipLaunchKernelGGL(k_sel_finish, dim3(1), dim3(256), 0, s, w, fin);
    DGC_LAUNCHED();
    return DGC_OK;
}

// ------------------------------------------------------------------ host tables, workspace
// What build_layout derives from a call's tensor list, held together.
struct HostTables {
    Layout L;
    std::vector<TDesc> td;
    std::vector<int32_t> bt[BT_COUNT], small;
    void build(const TensorIn* in, int32_t T, bool padded) { build_layout(in, T, padded, L, td, bt, small); }
};

// The workspace of a call, checked and carved. args_ok: a caller's own condition that
// reports with the workspace code (dgc_batch_flush's null vec / mmt).
static int carve_checked(void* ws, size_t ws_bytes, const Layout& L, const char* who, SelWS& w, bool args_ok = true) {
    size_t need = 0;
    carve_select(nullptr, L, &need);
    if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 255) || !args_ok)
        DGC_FAIL(DGC_ERR_WORKSPACE, "%s: workspace needs %zu bytes, 256-B aligned", who, need);
    w = carve_select(ws, L);
    return DGC_OK;
}

// ------------------------------------------------------------------ one-tensor plumbing
// Layout + table of one unpadded tensor. samples: reserve the strided-sample buffer.
static void one_layout(const dgc_select_params& p, int64_t stride, int64_t ks, bool samples, Layout& L,
                       OneTable& ot) {
    TensorIn in{p.numel, 0, p.num_selects, p.num_samples, ks, stride, p.upper_count, p.lower_count, samples};
    HostTables h;
    h.build(&in, 1, false);
    L = h.L;
    ot.d = h.td[0];
    for (int which = 0; which < BT_COUNT; ++which) {
        ot.bt[which][0] = h.bt[which][0];
        ot.bt[which][1] = h.bt[which][1];
    }
    ot.start = 0;
}

static size_t one_ws_bytes(int64_t numel, int64_t k, int64_t num_samples, bool samples) {
    dgc_select_params p{};
    p.numel = numel;
    p.num_selects = k;
    p.num_samples = num_samples;
    Layout L;
    OneTable ot{};
    one_layout(p, 2, 1, samples, L, ot);
    size_t b = 0;
    carve_select(nullptr, L, &b);
    return b;
}

static size_t select_ws_bytes(int64_t numel, int64_t k) { return one_ws_bytes(numel, k, numel, false); }

int select(float* vec, float* mmt, const float* thr0, const dgc_select_params* p, void* values, void* indices,
           int64_t* count_out, dgc_select_info* info, void* ws, size_t ws_bytes, int sync_mode, hipStream_t s) {
    DGC_TRY(validate_select(p, values, indices));
    if (!vec || !thr0 || (p->update_memory && p->masking && !mmt))
        DGC_FAIL(DGC_ERR_INVALID, "dgc_select: null vec/thr0/mmt");
    Layout L;
    OneTable ot{};
    one_layout(*p, 1, 1, false, L, ot);
    SelWS w;
    DGC_TRY(carve_checked(ws, ws_bytes, L, "dgc_select", w));
    w.spec = nullptr;
    w.thr = const_cast<float*>(thr0);
    hipLaunchKernelGGL(k_put_one, dim3(1), dim3(64), 0, s, w, ot);
    DGC_LAUNCHED();
    return select_core(vec, mmt, cfg_of(*p), L, values, indices, count_out, info, w, 0, sync_mode, 1.f,
                       p->status_sink, p->order_out, s);
}

// ------------------------------------------------------------------ threshold
static size_t kth_ws_bytes(int64_t n) { return n <= kSmallN ? 256 : align_up(sizeof(RSState), 256); }

int kth_largest(const float* x, int64_t n, int64_t k, float* out, void* ws, size_t ws_bytes, hipStream_t s) {
    if (!x || !out || n < 1 || k < 1 || k > n)
        DGC_FAIL(DGC_ERR_INVALID, "dgc_kth_largest: need 1 <= k <= n (k=%lld n=%lld)", (long long)k,
                 (long long)n);
    if (n <= kSmallN) {
        hipLaunchKernelGGL(k_rs_small, dim3(1), dim3(kScanThreads), 0, s, x, n, (uint64_t)k, out);
        DGC_LAUNCHED();
        return DGC_OK;
    }
    if (!ws || ws_bytes < sizeof(RSState) || (reinterpret_cast<uintptr_t>(ws) & 255))
        DGC_FAIL(DGC_ERR_WORKSPACE, "dgc_kth_largest: workspace needs %zu bytes", sizeof(RSState));
    RSState* st = reinterpret_cast<RSState*>(ws);
    hipLaunchKernelGGL(k_rs_init, dim3(1), dim3(kBlock), 0, s, st, (uint64_t)k);
    DGC_LAUNCHED();
    return radix_select_passes(DenseKeys{x, n, st, out}, grid_for(n, kBlock * 16, 512), s);
}

// K3 of every tensor of the call: the small ones in one workgroup each, the rest in
// three multi-block passes.
static int thresholds(const SelWS& w, const Layout& L, const float* vec, hipStream_t s, int64_t ks1 = 0) {
    if (L.nsmall + L.nwins) {
        hipLaunchKernelGGL(k_rs_small_multi, dim3((unsigned)(L.nsmall + L.nwins)), dim3(kScanThreads), 0, s, w, vec,
                           ks1, L.nsmall);
        DGC_LAUNCHED();
    }
    if (L.grid[BT_SAMP] > 0) {
        if (L.nplain) {   // (a windowed task's reset is k_rs_small_multi's)
            hipLaunchKernelGGL(k_rs_reset_samples, dim3((unsigned)L.T), dim3(kBlock), 0, s, w, ks1);
            DGC_LAUNCHED();
        }
        const int grid = (int)L.grid[BT_SAMP];
        hipLaunchKernelGGL(k_rs_passes<SampleKeys>, dim3((unsigned)std::min(grid, 1024)), dim3(kBlock), 0, s,
                           SampleKeys{w, vec}, grid, (int)L.T);
        DGC_LAUNCHED();
    }
    return DGC_OK;
}

// ------------------------------------------------------------------ fused compress (one tensor)
int compensate(const float* grad, float* mmt, float* vec, float* out, int64_t n, float momentum,
               bool nesterov, bool accumulate, float* samples, int64_t s_start, int64_t s_stride,
               int64_t s_count, hipStream_t st);
int compensate_clip(const float* grad, float* mmt, float* vec, float* out, int64_t n, float momentum,
                    bool nesterov, bool accumulate, float* samples, int64_t s_start, int64_t s_stride,
                    int64_t s_count, int32_t clip_kind, ClipArg ca, hipStream_t st);
int sample_strided_launch(const float* vec, int64_t start, int64_t stride, int64_t count, float* out,
                          hipStream_t s);

static int compress_check(const dgc_select_params* p, void* values, void* indices, int64_t s_start,
                          int64_t s_stride, int64_t top_k_samples, bool need_outputs) {
    if (need_outputs) DGC_TRY(validate_select(p, values, indices));
    else if (!p) DGC_FAIL(DGC_ERR_INVALID, "dgc_compress: null params");
    else if (p->resample) DGC_TRY(check_replay_width(p->numel, p->num_selects, "dgc_compress"));
    const bool sampled = p->numel != p->num_samples;
    if (sampled && (s_stride < 2 || s_start < 0 || s_start >= s_stride))
        DGC_FAIL(DGC_ERR_INVALID, "dgc_compress: sample_start must be in [0, stride)");
    const int64_t cnt = sampled ? ceil_div(p->numel - s_start, s_stride) : p->numel;
    if (need_outputs && (top_k_samples < 1 || top_k_samples > cnt))
        DGC_FAIL(DGC_ERR_INVALID, "dgc_compress: top_k_samples %lld outside [1, %lld]", (long long)top_k_samples,
                 (long long)cnt);
    return DGC_OK;
}

static int one_ws(const dgc_select_params* p, int64_t s_start, int64_t s_stride, int64_t ks, float* spec,
                  void* ws, size_t ws_bytes, Layout& L, SelWS& w, OneTable& ot) {
    one_layout(*p, s_stride, ks, true, L, ot);
    ot.start = p->numel != p->num_samples ? s_start : 0;
    DGC_TRY(carve_checked(ws, ws_bytes, L, "dgc_compress", w));
    w.spec = spec;   // the caller's per-tensor float[kSpecWords] (null: no speculative lists)
    return DGC_OK;
}

// K1 (+ fused strided sample + speculative candidate lists at spec[0]).
// clip_kind / ca: the gradient clipped as K1 loads it (dgc_compress_begin_clip).
// lds: bytes of LDS the launch asks for and the kernel never touches, which bounds how many
// workgroups a CU holds. A one-tensor call (the flat bucket) past the write-through size
// asks for kK1FlatLds: 3 workgroups then fit a CU's 160 KB, 3 waves per SIMD with 12 KB of
// loads in flight each. K1's registers allow 6-7 waves, and flat-1B measured slower the more
// of them were resident (same box, K1 ms: 7 waves 3.44-3.49, 5 waves 3.43, 4 waves
// 3.24-3.42, 3 waves 3.19-3.41, 2 waves 3.48; DESIGN.md §5 "K1's schedule"). Every other
// launch — a batch, a bucket of at most kWriteThroughMax elements — keeps the
// register-limited occupancy: the model sets measured faster with it, and no small flat
// bucket was measured either way.
constexpr unsigned kK1FlatLds = 48u << 10;

// The sample strides the listing kernels (K1, K1-16) take: a lane's 4 elements hold at most
// one sample (stride >= 4), and the per-tile sample's divmod (k1_sample) runs in 32 bits
// (stride < 2^30). With 16-B alignment of the arrays, the whole condition under which a
// tensor can take them.
static bool k1_stride_ok(bool sampled, int64_t stride) { return !sampled || (stride >= 4 && stride < (1LL << 30)); }

// The samples that fall into an unpadded tensor's scalar tail [done, n), read back from vec
// once the tail is compensated: start + q * stride >= done. cnt: the tensor's sample count.
static int sample_tail(const float* vec, int64_t done, int64_t s_start, int64_t s_stride, int64_t cnt, float* samples,
                       hipStream_t s) {
    const int64_t q_first = done >= s_start ? ceil_div(done - s_start, s_stride) : 0;
    const int64_t c = cnt - q_first;
    if (c <= 0) return DGC_OK;
    return sample_strided_launch(vec, s_start + q_first * s_stride, s_stride, c, samples + q_first, s);
}

// K1 of one tensor (ONE: the flat bucket) or of a batch; the two callers differ in the tables they pass.
// gdt: the gradient's dtype. A 16-bit one (DGC_BF16 / DGC_F16) is the flat bucket's alone, unclipped.
template <bool ONE, typename... Args>
static void launch_k1(int32_t gdt, bool nesterov, int32_t clip_kind, unsigned lds, dim3 gd, hipStream_t s,
                      const void* grad, Args... args) {
    with_bool(nesterov, [&](auto NEST) {
        if (gdt == DGC_F32) {
            with_clip(clip_kind, [&](auto CLIP) {
                hipLaunchKernelGGL((k_compensate_list<NEST(), ONE, CLIP()>), gd, dim3(kBlock), lds, s,
                                   static_cast<const float*>(grad), args...); });
        } else if constexpr (ONE) {
            with_h16(gdt, [&](auto GD) {
                hipLaunchKernelGGL((k_compensate_list<NEST(), true, DGC_CLIP_NONE, GD()>), gd, dim3(kBlock), lds, s,
                                   static_cast<const uint16_t*>(grad), args...); });
        }
    });
}

// The list path of a one-tensor call (the flat bucket), fp32 state under a gradient of dtype
// gdt: the workspace, K1 with the tensor's tables and sample start in its arguments, and the
// scalar tail of the unpadded tensor. A 16-bit gradient is unclipped and has no k_put_one
// path: its caller (who) refuses what yields no K1 workgroup.
static int one_k1(const char* who, const void* grad, int32_t gdt, float* mmt, float* vec, float momentum,
                  bool nesterov, int64_t s_start, int64_t s_stride, const dgc_select_params* p, float* spec, void* ws,
                  size_t ws_bytes, int32_t clip_kind, ClipArg ca, hipStream_t s) {
    Layout L;
    SelWS w;
    OneTable ot{};
    DGC_TRY(one_ws(p, s_start, s_stride, 1, spec, ws, ws_bytes, L, w, ot));
    const bool f32 = gdt == DGC_F32;
    const int64_t n = p->numel;
    const bool sampled = n != p->num_samples;
    if (L.grid[BT_K1] > 0x7FFFFFFFLL || (!f32 && L.grid[BT_K1] < 1)) DGC_FAIL(DGC_ERR_INVALID, "%s: n too large", who);
    if (L.grid[BT_K1] > 0) {
        StartChunk one{};   // the start (and the tables, ot) in the arguments: no k_put_one
        one.count = 1;
        one.start[0] = ot.start;
        // a 16-bit gradient keeps the fp32 launch's occupancy policy: 10 of its 12 KB in flight per wave
        const bool wt = write_through(n);
        launch_k1<true>(gdt, nesterov, clip_kind, wt ? 0u : kK1FlatLds, dim3((unsigned)L.grid[BT_K1]), s, grad, mmt, vec,
                        momentum, w, one, (int)wt, ot, ca);
        DGC_LAUNCHED();
    } else {
        hipLaunchKernelGGL(k_put_one, dim3(1), dim3(64), 0, s, w, ot);
        DGC_LAUNCHED();
    }
    if (n & 3) {   // scalar tail (< 4 elements) incl. its samples; its segment is marked spilled
        const int64_t done = (n / 4) * 4;
        if (f32) {
            DGC_TRY(compensate_clip(static_cast<const float*>(grad) + done, mmt + done, vec + done, nullptr, n - done,
                                    momentum, nesterov, true, nullptr, 0, 1, 0, clip_kind, ca, s));
        } else {
            with_h16(gdt, [&](auto GD) { with_bool(nesterov, [&](auto NEST) {
                hipLaunchKernelGGL((k_compensate_tail_g16<GD(), NEST()>), dim3(1), dim3(64), 0, s,
                                   static_cast<const uint16_t*>(grad), mmt, vec, done, n, momentum); }); });
            DGC_LAUNCHED();
        }
        if (sampled) DGC_TRY(sample_tail(vec, done, s_start, s_stride, ceil_div(n - s_start, s_stride), w.samples, s));
    }
    return DGC_OK;
}

int compress_begin(const float* grad, float* mmt, float* vec, float momentum, bool nesterov, int64_t s_start,
                   int64_t s_stride, const dgc_select_params* p, float* spec, void* ws, size_t ws_bytes,
                   hipStream_t s, int32_t clip_kind = DGC_CLIP_NONE, ClipArg ca = ClipArg{nullptr, 0.f}) {
    DGC_TRY(compress_check(p, nullptr, nullptr, s_start, s_stride, 1, false));
    DGC_TRY(check_clip("dgc_compress", clip_kind, ca.tab));
    if (!grad || !mmt || !vec) DGC_FAIL(DGC_ERR_INVALID, "dgc_compress: null grad/mmt/vec");
    const int64_t n = p->numel;
    const bool sampled = n != p->num_samples;
    if (aligned16(grad) && aligned16(mmt) && aligned16(vec) && k1_stride_ok(sampled, s_stride))
        return one_k1("dgc_compress", grad, DGC_F32, mmt, vec, momentum, nesterov, s_start, s_stride, p, spec, ws,
                      ws_bytes, clip_kind, ca, s);
    // the unfused fallback: no lists
    Layout L;
    SelWS w;
    OneTable ot{};
    DGC_TRY(one_ws(p, s_start, s_stride, 1, spec, ws, ws_bytes, L, w, ot));
    hipLaunchKernelGGL(k_put_one, dim3(1), dim3(64), 0, s, w, ot);
    DGC_LAUNCHED();
    DGC_TRY(mask_flush(vec, mmt, L, w, s));   // a deferring finish left its masking to K1
    DGC_TRY(compensate_clip(grad, mmt, vec, nullptr, n, momentum, nesterov, true, sampled ? w.samples : nullptr, s_start,
                            s_stride, sampled ? ceil_div(n - s_start, s_stride) : 0, clip_kind, ca, s));
    hipLaunchKernelGGL(k_no_lists, dim3(1), dim3(64), 0, s, w);
    DGC_LAUNCHED();
    return DGC_OK;
}

// K1 of the flat bucket with fp32 momentum / velocity and a bf16 / fp16 gradient, widened in
// K1's load (k_compensate_list's GD): compress_begin on the widened gradient without the
// widened copy, so dgc_compress_finish and dgc_compress_flush follow as they follow
// compress_begin. Unclipped, and with no unfused fallback: what the listing kernel cannot
// take is refused here, the rest is compress_begin's list path (one_k1).
int compress_begin_g16(const void* grad, int32_t grad_dtype, float* mmt, float* vec, float momentum, bool nesterov,
                       int64_t s_start, int64_t s_stride, const dgc_select_params* p, float* spec, void* ws,
                       size_t ws_bytes, hipStream_t s) {
    const char* who = "dgc_compress_begin_g16";
    if (!is16(grad_dtype))
        DGC_FAIL(DGC_ERR_DTYPE, "%s: grad_dtype must be DGC_BF16 or DGC_F16 (got %d)", who, (int)grad_dtype);
    if (!grad || !mmt || !vec || !p) DGC_FAIL(DGC_ERR_INVALID, "%s: null grad/mmt/vec/params", who);
    if (reinterpret_cast<uintptr_t>(grad) & 7u) DGC_FAIL(DGC_ERR_INVALID, "%s: grad must be 8-B aligned", who);
    if (!aligned16(mmt) || !aligned16(vec)) DGC_FAIL(DGC_ERR_INVALID, "%s: mmt and vec must be 16-B aligned", who);
    if (!k1_stride_ok(p->numel != p->num_samples, s_stride))
        DGC_FAIL(DGC_ERR_INVALID, "%s: sample stride %lld outside [4, 2^30)", who, (long long)s_stride);
    DGC_TRY(compress_check(p, nullptr, nullptr, s_start, s_stride, 1, false));
    return one_k1(who, grad, grad_dtype, mmt, vec, momentum, nesterov, s_start, s_stride, p, spec, ws, ws_bytes,
                  DGC_CLIP_NONE, ClipArg{nullptr, 0.f}, s);
}

// K1-16 of the flat bucket: 16-bit momentum / velocity / gradient, the velocity's fp32
// image vec32 (+ fused strided sample + speculative candidate lists, all from the image);
// dgc_compress_finish(vec32, null, ...) then serves the image. mmt, vec and vec32 hold
// ceil(numel / 1024) * 1024 elements. There is no unfused fallback: what the listing
// kernel cannot take is refused.
int compress_begin16(const void* grad, void* mmt, void* vec, float* vec32, float momentum, bool nesterov,
                     int64_t s_start, int64_t s_stride, const dgc_select_params* p, float* spec, void* ws,
                     size_t ws_bytes, int32_t dtype, hipStream_t s, int32_t clip_kind = DGC_CLIP_NONE,
                     ClipArg ca = ClipArg{nullptr, 0.f}, const char* who = "dgc_compress_begin16") {
    if (!is16(dtype)) DGC_FAIL(DGC_ERR_INVALID, "%s: dtype must be DGC_BF16 or DGC_F16 (got %d)", who, (int)dtype);
    if (!grad || !mmt || !vec || !vec32 || !p)
        DGC_FAIL(DGC_ERR_INVALID, "%s: null grad/mmt/vec/vec32/params", who);
    DGC_TRY(check_clip(who, clip_kind, ca.tab));
    if (p->update_memory != 0)
        DGC_FAIL(DGC_ERR_INVALID, "%s: update_memory must be 0 (the 16-bit state is masked from "
                                  "the payload, dgc_mask_packed16)", who);
    if (p->thr_dtype != dtype)
        DGC_FAIL(DGC_ERR_INVALID, "%s: params.thr_dtype %d must be the dtype %d", who, (int)p->thr_dtype,
                 (int)dtype);
    DGC_TRY(compress_check(p, nullptr, nullptr, s_start, s_stride, 1, false));
    const int64_t n = p->numel;
    const bool sampled = n != p->num_samples;
    if (!aligned16(grad) || !aligned16(mmt) || !aligned16(vec) || !aligned16(vec32))
        DGC_FAIL(DGC_ERR_INVALID, "%s: grad, mmt, vec and vec32 must be 16-B aligned", who);
    if (!k1_stride_ok(sampled, s_stride))
        DGC_FAIL(DGC_ERR_INVALID, "%s: sample stride %lld outside [4, 2^30)", who, (long long)s_stride);
    Layout L;
    SelWS w;
    OneTable ot{};
    DGC_TRY(one_ws(p, s_start, s_stride, 1, spec, ws, ws_bytes, L, w, ot));
    if (L.grid[BT_K1] < 1 || L.grid[BT_K1] > 0x7FFFFFFFLL)
        DGC_FAIL(DGC_ERR_INVALID, "%s: n too large", who);
    // No kK1FlatLds here: a wave of this kernel has 6 KB of loads in flight where the fp32
    // one has 12, and held to 3 waves per SIMD it ran slower. Same box, 1e9 elements, K1-16
    // ms: 3 waves (48 KB of LDS asked for) 2.47-2.49, 6 waves (24 KB) 2.28, the registers'
    // 7 waves 2.28; two segments per wave (24 loads in flight) 2.42 / 2.33 / 2.33 at the
    // same three (DESIGN.md §5 "The 16-bit flat bucket").
    const bool wt = write_through(n);
    const dim3 gd((unsigned)L.grid[BT_K1]);
    const uint16_t* g16 = static_cast<const uint16_t*>(grad);
    uint16_t *m16 = static_cast<uint16_t*>(mmt), *v16 = static_cast<uint16_t*>(vec);
    with_h16(dtype, [&](auto DT) { with_bool(nesterov, [&](auto NEST) { with_clip(clip_kind, [&](auto CLIP) {
        hipLaunchKernelGGL((k_compensate_list16<DT(), NEST(), CLIP()>), gd, dim3(kBlock), 0, s, g16, m16, v16, vec32, momentum,
                           w, ot.start, (int)wt, ot, ca); }); }); });
    DGC_LAUNCHED();
    return DGC_OK;
}

// K3 threshold over the samples, then the selection (lists kept from begin).
int compress_finish(float* vec, float* mmt, int64_t s_start, int64_t s_stride, int64_t top_k_samples,
                    const dgc_select_params* p, float* spec, float margin, void* values, void* indices,
                    int64_t* count_out, dgc_select_info* info, void* ws, size_t ws_bytes, int sync_mode,
                    hipStream_t s) {
    DGC_TRY(compress_check(p, values, indices, s_start, s_stride, top_k_samples, true));
    // update_memory 0 with masking set and no momentum to mask: the pure selection of a
    // 16-bit bucket's fp32 image (dgc_compress_begin16), which writes neither vec nor mmt
    const bool pure = p->update_memory == 0 && p->masking && !mmt;
    if (!vec || (p->masking && !mmt && !pure)) DGC_FAIL(DGC_ERR_INVALID, "dgc_compress: null vec/mmt");
    Layout L;
    SelWS w;
    OneTable ot{};
    DGC_TRY(one_ws(p, s_start, s_stride, top_k_samples, spec, ws, ws_bytes, L, w, ot));
    // the table dgc_compress_begin wrote serves as is (the layout does not depend on
    // top_k_samples); K3 gets top_k_samples in its arguments
    DGC_TRY(thresholds(w, L, vec, s, top_k_samples));
    dgc_select_params q = *p;
    // DGCSGDMemory.update fused into the emit (1), or deferred into the next K1 (2)
    q.update_memory = pure ? 0 : (p->update_memory == 2 ? 2 : 1);
    return select_core(vec, mmt, cfg_of(q), L, values, indices, count_out, info, w, 1, sync_mode, margin,
                       p->status_sink, p->order_out, s);
}

// ------------------------------------------------------------------ batch
static int batch_layout(const dgc_batch_desc* b, HostTables& h) {
    if (!b || b->count < 1 || !b->numel || !b->offset || !b->num_selects || !b->num_samples || !b->top_k_samples ||
        !b->sample_stride)
        DGC_FAIL(DGC_ERR_INVALID, "dgc_batch: null or empty tensor table");
    std::vector<TensorIn> in(b->count);
    int64_t prev_end = 0;
    for (int32_t t = 0; t < b->count; ++t) {
        TensorIn& x = in[t];
        x.n = b->numel[t];
        x.off = b->offset[t];
        x.k = b->num_selects[t];
        x.S = b->num_samples[t];
        x.ks = b->top_k_samples[t];
        x.stride = b->sample_stride[t];
        x.upper_count = (int64_t)std::floor((double)x.k * b->upper_bound);
        x.lower_count = (int64_t)std::ceil(b->lower_bound * (double)x.k);
        x.samples = true;
        if (x.n < 1 || x.k < 1 || x.k > x.n || x.S < 1 || x.S > x.n || x.ks < 1 || x.ks > x.S)
            DGC_FAIL(DGC_ERR_INVALID, "dgc_batch: tensor %d: bad numel/num_selects/num_samples/top_k_samples", t);
        if (b->resample) {
            char who[48];
            std::snprintf(who, sizeof(who), "dgc_batch: tensor %d", t);
            DGC_TRY(check_replay_width(x.n, x.k, who));
        }
        if (!k1_stride_ok(x.n != x.S, x.stride))
            DGC_FAIL(DGC_ERR_INVALID, "dgc_batch: tensor %d: sample stride %lld outside [4, 2^30)", t,
                     (long long)x.stride);
        if (x.off % kSeg || x.off < prev_end)
            DGC_FAIL(DGC_ERR_INVALID,
                     "dgc_batch: tensor %d: offset %lld must be a multiple of %d, ascending, non-overlapping", t,
                     (long long)x.off, kSeg);
        prev_end = x.off + (int64_t)align_up((size_t)x.n, 4);
        if (prev_end > b->flat_numel) DGC_FAIL(DGC_ERR_INVALID, "dgc_batch: tensor %d past flat_numel", t);
    }
    if (b->int32_indices && b->flat_numel > 2147483647LL)
        DGC_FAIL(DGC_ERR_OVERFLOW, "dgc_batch: int32 indices cannot address %lld elements", (long long)b->flat_numel);
    if (!float_dtype_ok(b->dtype))
        DGC_FAIL(DGC_ERR_DTYPE, "dgc_batch: dtype must be DGC_F32, DGC_BF16 or DGC_F16");
    h.build(in.data(), b->count, true);
    return DGC_OK;
}

// A 16-bit batch (dtype bf16 / fp16) selects on the velocities' fp32 image without
// touching it (update_memory 0; the 16-bit state is masked from the payload,
// dgc_mask_packed16), its wire values in the parameter dtype unless fp16_values, and its
// threshold *= bound products rounded to the dtype.
static SelCfg cfg_of_batch(const dgc_batch_desc* b) {
    const bool half = is16(b->dtype);
    return SelCfg{(float)b->upper_bound, (float)b->lower_bound, b->max_iters, b->resample, b->momentum_masking,
                  b->fp16_values ? DGC_F16 : (half ? b->dtype : DGC_F32), b->int32_indices ? DGC_I32 : DGC_I64,
                  half ? 0 : (b->deferred_masking ? 2 : 1), half ? b->dtype : DGC_F32,
                  b->resample_order == 1 ? 1 : 0};
}

// Host layout + workspace check shared by the batch entry points.
static int batch_ws(const dgc_batch_desc* b, void* ws, size_t ws_bytes, const char* who, HostTables& h, SelWS& w,
                    bool args_ok = true) {
    DGC_TRY(batch_layout(b, h));
    return carve_checked(ws, ws_bytes, h.L, who, w, args_ok);
}

size_t batch_ws_bytes(const dgc_batch_desc* b) {
    HostTables h;
    if (batch_layout(b, h) != DGC_OK) return 0;
    size_t n = 0;
    carve_select(nullptr, h.L, &n);
    return n;
}

int batch_init(const dgc_batch_desc* b, void* ws, size_t ws_bytes, hipStream_t s) {
    HostTables h;
    SelWS w;
    DGC_TRY(batch_ws(b, ws, ws_bytes, "dgc_batch_init", h, w));
    const Layout& L = h.L;
    DGC_HIP(hipMemsetAsync(w.st, 0, sizeof(SelState) * L.T, s));
    DGC_HIP(hipMemsetAsync(w.setg, 0, sizeof(SetG) * L.T, s));                         // zero at rest
    DGC_HIP(hipMemsetAsync(w.chain, 0, kChainWords * sizeof(uint32_t), s));            // zero at rest
    DGC_HIP(hipMemsetAsync(w.samples, 0, sizeof(float) * L.nsamp, s));   // the window histograms: zero at rest
    DGC_HIP(hipMemcpyAsync(w.td, h.td.data(), sizeof(TDesc) * L.T, hipMemcpyHostToDevice, s));
    for (int which = 0; which < BT_COUNT; ++which)
        DGC_HIP(hipMemcpyAsync(w.bt[which], h.bt[which].data(), sizeof(int32_t) * (L.T + 1), hipMemcpyHostToDevice, s));
    if (L.nsmall + L.nwins)
        DGC_HIP(hipMemcpyAsync(w.small, h.small.data(), sizeof(int32_t) * (L.nsmall + L.nwins),
                               hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_spec_reset, dim3(1), dim3(256), 0, s, w.spec, L.T);
    DGC_LAUNCHED();
    // the host tables are pageable and local: let the copies finish first
    DGC_HIP(hipStreamSynchronize(s));
    return DGC_OK;
}

// A call's sample starts, checked: inside [0, stride) for every sampled tensor.
static int check_starts(const HostTables& h, const int64_t* starts, const char* who) {
    for (int32_t t = 0; t < h.L.T; ++t)
        if (h.td[t].samp_off >= 0 && (starts[t] < 0 || starts[t] >= h.td[t].stride))
            DGC_FAIL(DGC_ERR_INVALID, "%s: tensor %d: sample start outside [0, stride)", who, t);
    return DGC_OK;
}

// The starts (0 for an unsampled tensor) and gradient pointers of up to 64 tensors from `first`.
static StartChunk start_chunk(const HostTables& h, const int64_t* starts, const float* const* grads, int32_t first) {
    StartChunk c{};
    c.first = first;
    c.count = std::min<int32_t>(64, h.L.T - first);
    c.ptrs = grads ? 1 : 0;
    for (int i = 0; i < c.count; ++i) {
        c.start[i] = h.td[first + i].samp_off >= 0 ? starts[first + i] : 0;
        c.grad[i] = grads ? grads[first + i] : nullptr;
    }
    return c;
}

static int put_starts(const HostTables& h, const int64_t* starts, const float* const* grads, const SelWS& w,
                      hipStream_t s) {
    for (int32_t t0 = 0; t0 < h.L.T; t0 += 64) {
        hipLaunchKernelGGL(k_put_starts, dim3(1), dim3(64), 0, s, w, start_chunk(h, starts, grads, t0));
        DGC_LAUNCHED();
    }
    return DGC_OK;
}

// The payload split, then the selection of every tensor into the one packed payload.
static int batch_select_core(const dgc_batch_desc* b, const SelCfg& cfg, const HostTables& h, float* vec, float* mmt,
                             void* payload, dgc_select_info* info, const SelWS& w, int sync_mode, hipStream_t s) {
    int64_t cap = 0;
    for (const TDesc& d : h.td) cap += d.k;
    int64_t voff = 0, ioff = 0;
    payload_layout(cap, cfg.vdtype, cfg.idtype, &voff, &ioff);
    char* pl = static_cast<char*>(payload);
    return select_core(vec, mmt, cfg, h.L, pl + voff, pl + ioff, reinterpret_cast<int64_t*>(pl), info, w, 1,
                       sync_mode, b->spec_margin, b->status_sink, reinterpret_cast<int64_t*>(pl) + 1, s);
}

// K1 over every tensor (+ fused strided samples + speculative candidate lists), the
// gradients from the flat buffer (grads == null) or from a host table of T device
// pointers (grads[t]: numel[t] contiguous floats, 16-B aligned).
int batch_compress_begin(const dgc_batch_desc* b, const float* grad, const float* const* grads, float* mmt,
                         float* vec, const int64_t* starts, void* ws, size_t ws_bytes, hipStream_t s,
                         int32_t clip_kind = DGC_CLIP_NONE, ClipArg ca = ClipArg{nullptr, 0.f}) {
    HostTables h;
    SelWS w;
    DGC_TRY(check_clip("dgc_batch_compress", clip_kind, ca.tab));
    DGC_TRY(batch_ws(b, ws, ws_bytes, "dgc_batch_compress", h, w));
    const Layout& L = h.L;
    if ((!grad && !grads) || !mmt || !vec || !starts) DGC_FAIL(DGC_ERR_INVALID, "dgc_batch_compress: null pointer");
    if ((grad && !aligned16(grad)) || !aligned16(mmt) || !aligned16(vec))
        DGC_FAIL(DGC_ERR_INVALID, "dgc_batch_compress: flat buffers must be 16-B aligned");
    if (grads)
        for (int32_t t = 0; t < L.T; ++t)
            if (!grads[t] || !aligned16(grads[t]))
                DGC_FAIL(DGC_ERR_INVALID, "dgc_batch_compress: gradient %d is null or not 16-B aligned", t);
    DGC_TRY(check_starts(h, starts, "dgc_batch_compress"));
    // up to 64 starts go to K1 in its arguments; a larger batch puts them first
    StartChunk arg{};
    arg.ptrs = grads ? 1 : 0;
    if (L.T <= 64) arg = start_chunk(h, starts, grads, 0);
    else DGC_TRY(put_starts(h, starts, grads, w, s));
    if (L.grid[BT_K1] > 0x7FFFFFFFLL) DGC_FAIL(DGC_ERR_INVALID, "dgc_batch_compress: too many segments");
    launch_k1<false>(DGC_F32, b->nesterov != 0, clip_kind, 0u, dim3((unsigned)L.grid[BT_K1]), s, grad, mmt, vec, b->momentum,
                     w, arg, (int)write_through(L.nseg * kSeg), OneTable{}, ca);
    DGC_LAUNCHED();
    return DGC_OK;
}

// K3 thresholds, then the selection of every tensor into the one packed payload.
int batch_compress_finish(const dgc_batch_desc* b, float* mmt, float* vec, void* payload, dgc_select_info* info,
                          void* ws, size_t ws_bytes, int sync_mode, hipStream_t s) {
    HostTables h;
    SelWS w;
    DGC_TRY(batch_ws(b, ws, ws_bytes, "dgc_batch_compress", h, w));
    if (!mmt || !vec || !payload) DGC_FAIL(DGC_ERR_INVALID, "dgc_batch_compress: null pointer");
    DGC_TRY(thresholds(w, h.L, vec, s));
    return batch_select_core(b, cfg_of_batch(b), h, vec, mmt, payload, info, w, sync_mode, s);
}

// The strided samples |x[start + q * stride]| of every sampled tensor from a flat fp32
// buffer (K1 writes them on the fp32 path); grid: (chunks, T).
__global__ void __launch_bounds__(kBlock) k_batch_sample(SelWS w, const float* __restrict__ x_flat) {
    const int t = blockIdx.y;
    const TDesc d = w.td[t];
    if (d.samp_off < 0) return;
    const int64_t start = w.starts[t], cnt = w.scnt[t];
    const float* x = x_flat + d.off + start;
    float* out = w.samples + d.samp_off;
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < cnt; q += (int64_t)gridDim.x * kBlock)
        out[q] = fabsf(x[q * d.stride]);
}

// The selection of a batch over a flat fp32 buffer vec32 that no K1 of this library
// produced (a 16-bit batch's velocity image, dgc_compensate16): the strided samples,
// then dgc_batch_compress_finish's thresholds and selection (no candidate lists: the
// first count is a full pass). With dtype = DGC_F32 and update_memory (the desc's
// deferred_masking off) it masks vec32 like the fused path; a 16-bit batch never
// writes vec32.
int batch_select(const dgc_batch_desc* b, float* vec32, float* mmt32, const int64_t* starts, void* payload,
                 dgc_select_info* info, void* ws, size_t ws_bytes, int sync_mode, hipStream_t s) {
    HostTables h;
    SelWS w;
    DGC_TRY(batch_ws(b, ws, ws_bytes, "dgc_batch_select", h, w));
    const Layout& L = h.L;
    if (!vec32 || !starts || !payload) DGC_FAIL(DGC_ERR_INVALID, "dgc_batch_select: null pointer");
    const SelCfg cfg = cfg_of_batch(b);
    if (cfg.update_memory && cfg.masking && !mmt32) DGC_FAIL(DGC_ERR_INVALID, "dgc_batch_select: masking needs mmt");
    DGC_TRY(check_starts(h, starts, "dgc_batch_select"));
    DGC_TRY(put_starts(h, starts, nullptr, w, s));
    int64_t smax = 0;
    for (const TDesc& d : h.td) smax = std::max(smax, d.samp_off >= 0 ? d.S + 1 : 0);
    if (smax > 0) {
        hipLaunchKernelGGL(k_batch_sample, dim3((unsigned)std::min<int64_t>(ceil_div(smax, (int64_t)kBlock), 1024),
                                                (unsigned)L.T), dim3(kBlock), 0, s, w, vec32);
        DGC_LAUNCHED();
    }
    hipLaunchKernelGGL(k_no_lists, dim3(1), dim3(256), 0, s, w);   // t_list = +inf: no K1 lists
    DGC_LAUNCHED();
    DGC_TRY(thresholds(w, L, vec32, s));
    return batch_select_core(b, cfg, h, vec32, mmt32, payload, info, w, sync_mode, s);
}

int batch_compress(const dgc_batch_desc* b, const float* grad, float* mmt, float* vec, const int64_t* starts,
                   void* payload, dgc_select_info* info, void* ws, size_t ws_bytes, int sync_mode, hipStream_t s) {
    if (!payload) DGC_FAIL(DGC_ERR_INVALID, "dgc_batch_compress: null pointer");
    DGC_TRY(batch_compress_begin(b, grad, nullptr, mmt, vec, starts, ws, ws_bytes, s));
    return batch_compress_finish(b, mmt, vec, payload, info, ws, ws_bytes, sync_mode, s);
}

int compress_flush(float* vec, float* mmt, int64_t s_stride, const dgc_select_params* p, void* ws, size_t ws_bytes,
                   hipStream_t s) {
    if (!p || !vec) DGC_FAIL(DGC_ERR_INVALID, "dgc_compress_flush: null params/vec");
    Layout L;
    SelWS w;
    OneTable ot{};
    DGC_TRY(one_ws(p, 0, s_stride, 1, nullptr, ws, ws_bytes, L, w, ot));   // tables as the last call left them
    return mask_flush(vec, mmt, L, w, s);
}

int batch_flush(const dgc_batch_desc* b, float* mmt, float* vec, void* ws, size_t ws_bytes, hipStream_t s) {
    HostTables h;
    SelWS w;
    DGC_TRY(batch_ws(b, ws, ws_bytes, "dgc_batch_flush", h, w, vec && mmt));
    return mask_flush(vec, mmt, h.L, w, s);
}

}  // namespace dgc

// ------------------------------------------------------------------ C ABI
extern "C" size_t dgc_kth_largest_workspace(int64_t n) { return dgc::kth_ws_bytes(n); }

extern "C" int dgc_kth_largest(const float* x, int64_t n, int64_t k, float* thr_out, void* ws,
                               size_t ws_bytes, void* stream) {
    return dgc::kth_largest(x, n, k, thr_out, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" size_t dgc_select_workspace(int64_t numel, int64_t num_selects) {
    return dgc::select_ws_bytes(numel, num_selects);
}

extern "C" int dgc_select(float* vec, float* mmt, const float* thr0, const dgc_select_params* params,
                          void* values_out, void* indices_out, int64_t* count_out,
                          dgc_select_info* info_out, void* ws, size_t ws_bytes, int32_t sync_mode,
                          void* stream) {
    return dgc::select(vec, mmt, thr0, params, values_out, indices_out, count_out, info_out, ws, ws_bytes,
                       sync_mode, static_cast<hipStream_t>(stream));
}

extern "C" size_t dgc_compress_workspace(int64_t numel, int64_t num_selects, int64_t num_samples) {
    return dgc::one_ws_bytes(numel, num_selects, num_samples, true);
}

extern "C" int dgc_compress_begin(const float* grad, float* mmt, float* vec, float momentum, int32_t nesterov,
                                  int64_t sample_start, int64_t sample_stride, const dgc_select_params* params,
                                  const float* spec_threshold, void* ws, size_t ws_bytes, void* stream) {
    // begin only reads spec[0] (the list threshold); finish updates it
    return dgc::compress_begin(grad, mmt, vec, momentum, nesterov != 0, sample_start, sample_stride, params,
                               const_cast<float*>(spec_threshold), ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int dgc_compress_begin16(const void* grad, void* mmt, void* vec, float* vec32, float momentum,
                                    int32_t nesterov, int64_t sample_start, int64_t sample_stride,
                                    const dgc_select_params* params, const float* spec_threshold, void* ws,
                                    size_t ws_bytes, int32_t dtype, void* stream) {
    return dgc::compress_begin16(grad, mmt, vec, vec32, momentum, nesterov != 0, sample_start, sample_stride, params,
                                 const_cast<float*>(spec_threshold), ws, ws_bytes, dtype,
                                 static_cast<hipStream_t>(stream));
}

extern "C" int dgc_compress_begin16_clip(const void* grad, void* mmt, void* vec, float* vec32, float momentum,
                                         int32_t nesterov, int64_t sample_start, int64_t sample_stride,
                                         const dgc_select_params* params, const float* spec_threshold,
                                         int32_t clip_kind, const float* clip, float clip_value, void* ws,
                                         size_t ws_bytes, int32_t dtype, void* stream) {
    return dgc::compress_begin16(grad, mmt, vec, vec32, momentum, nesterov != 0, sample_start, sample_stride, params,
                                 const_cast<float*>(spec_threshold), ws, ws_bytes, dtype,
                                 static_cast<hipStream_t>(stream), clip_kind, dgc::ClipArg{clip, clip_value},
                                 "dgc_compress_begin16_clip");
}

extern "C" int dgc_compress_begin_g16(const void* grad, int32_t grad_dtype, float* mmt, float* vec, float momentum,
                                      int32_t nesterov, int64_t sample_start, int64_t sample_stride,
                                      const dgc_select_params* params, const float* spec_threshold, void* ws,
                                      size_t ws_bytes, void* stream) {
    return dgc::compress_begin_g16(grad, grad_dtype, mmt, vec, momentum, nesterov != 0, sample_start, sample_stride,
                                   params, const_cast<float*>(spec_threshold), ws, ws_bytes,
                                   static_cast<hipStream_t>(stream));
}

extern "C" int dgc_compress_finish(float* vec, float* mmt, int64_t sample_start, int64_t sample_stride,
                                   int64_t top_k_samples, const dgc_select_params* params, float* spec_threshold,
                                   float spec_margin, void* values_out, void* indices_out, int64_t* count_out,
                                   dgc_select_info* info_out, void* ws, size_t ws_bytes, int32_t sync_mode,
                                   void* stream) {
    return dgc::compress_finish(vec, mmt, sample_start, sample_stride, top_k_samples, params, spec_threshold,
                                spec_margin, values_out, indices_out, count_out, info_out, ws, ws_bytes,
                                sync_mode, static_cast<hipStream_t>(stream));
}

extern "C" int dgc_compress(const float* grad, float* mmt, float* vec, float momentum, int32_t nesterov,
                            int64_t sample_start, int64_t sample_stride, int64_t top_k_samples,
                            const dgc_select_params* params, float* spec_threshold, float spec_margin,
                            void* values_out, void* indices_out, int64_t* count_out, dgc_select_info* info_out,
                            void* ws, size_t ws_bytes, int32_t sync_mode, void* stream) {
    int rc = dgc::compress_begin(grad, mmt, vec, momentum, nesterov != 0, sample_start, sample_stride, params,
                                 spec_threshold, ws, ws_bytes, static_cast<hipStream_t>(stream));
    if (rc != DGC_OK) return rc;
    return dgc::compress_finish(vec, mmt, sample_start, sample_stride, top_k_samples, params, spec_threshold,
                                spec_margin, values_out, indices_out, count_out, info_out, ws, ws_bytes,
                                sync_mode, static_cast<hipStream_t>(stream));
}

extern "C" size_t dgc_batch_workspace(const dgc_batch_desc* batch) { return dgc::batch_ws_bytes(batch); }

extern "C" int dgc_batch_init(const dgc_batch_desc* batch, void* ws, size_t ws_bytes, void* stream) {
    return dgc::batch_init(batch, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int dgc_batch_compress(const dgc_batch_desc* batch, const float* grad, float* mmt, float* vec,
                                  const int64_t* sample_starts, void* payload, dgc_select_info* info_out, void* ws,
                                  size_t ws_bytes, int32_t sync_mode, void* stream) {
    return dgc::batch_compress(batch, grad, mmt, vec, sample_starts, payload, info_out, ws, ws_bytes, sync_mode,
                               static_cast<hipStream_t>(stream));
}

extern "C" int dgc_batch_compress_begin(const dgc_batch_desc* batch, const float* grad, float* mmt, float* vec,
                                        const int64_t* sample_starts, void* ws, size_t ws_bytes, void* stream) {
    return dgc::batch_compress_begin(batch, grad, nullptr, mmt, vec, sample_starts, ws, ws_bytes,
                                     static_cast<hipStream_t>(stream));
}

extern "C" int dgc_batch_select(const dgc_batch_desc* batch, float* vec32, float* mmt32, const int64_t* sample_starts,
                                void* payload, dgc_select_info* info_out, void* ws, size_t ws_bytes, int32_t sync_mode,
                                void* stream) {
    return dgc::batch_select(batch, vec32, mmt32, sample_starts, payload, info_out, ws, ws_bytes, sync_mode,
                             static_cast<hipStream_t>(stream));
}

extern "C" int dgc_batch_compress_begin_ptrs(const dgc_batch_desc* batch, const float* const* grads, float* mmt,
                                             float* vec, const int64_t* sample_starts, void* ws, size_t ws_bytes,
                                             void* stream) {
    if (!grads) DGC_FAIL(DGC_ERR_INVALID, "dgc_batch_compress_begin_ptrs: null gradient table");
    return dgc::batch_compress_begin(batch, nullptr, grads, mmt, vec, sample_starts, ws, ws_bytes,
                                     static_cast<hipStream_t>(stream));
}

extern "C" int dgc_compress_begin_clip(const float* grad, float* mmt, float* vec, float momentum, int32_t nesterov,
                                       int64_t sample_start, int64_t sample_stride, const dgc_select_params* params,
                                       const float* spec_threshold, int32_t clip_kind, const float* clip,
                                       float clip_value, void* ws, size_t ws_bytes, void* stream) {
    return dgc::compress_begin(grad, mmt, vec, momentum, nesterov != 0, sample_start, sample_stride, params,
                               const_cast<float*>(spec_threshold), ws, ws_bytes, static_cast<hipStream_t>(stream),
                               clip_kind, dgc::ClipArg{clip, clip_value});
}

extern "C" int dgc_batch_compress_begin_clip(const dgc_batch_desc* batch, const float* grad, float* mmt, float* vec,
                                             const int64_t* sample_starts, int32_t clip_kind, const float* clip,
                                             float clip_value, void* ws, size_t ws_bytes, void* stream) {
    return dgc::batch_compress_begin(batch, grad, nullptr, mmt, vec, sample_starts, ws, ws_bytes,
                                     static_cast<hipStream_t>(stream), clip_kind, dgc::ClipArg{clip, clip_value});
}

extern "C" int dgc_batch_compress_begin_ptrs_clip(const dgc_batch_desc* batch, const float* const* grads, float* mmt,
                                                  float* vec, const int64_t* sample_starts, int32_t clip_kind,
                                                  const float* clip, float clip_value, void* ws, size_t ws_bytes,
                                                  void* stream) {
    if (!grads) DGC_FAIL(DGC_ERR_INVALID, "dgc_batch_compress_begin_ptrs: null gradient table");
    return dgc::batch_compress_begin(batch, nullptr, grads, mmt, vec, sample_starts, ws, ws_bytes,
                                     static_cast<hipStream_t>(stream), clip_kind, dgc::ClipArg{clip, clip_value});
}

extern "C" int dgc_batch_compress_finish(const dgc_batch_desc* batch, float* mmt, float* vec, void* payload,
                                         dgc_select_info* info_out, void* ws, size_t ws_bytes, int32_t sync_mode,
                                         void* stream) {
    return dgc::batch_compress_finish(batch, mmt, vec, payload, info_out, ws, ws_bytes, sync_mode,
                                      static_cast<hipStream_t>(stream));
}

#ifdef DGC_K5_PROF
extern "C" int dgc_ce_prof(void* out) {
    DGC_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(dgc::g_ce_prof), sizeof(dgc::g_ce_prof)));
    return DGC_OK;
}

extern "C" int dgc_es_prof(void* out) {   // tools/es_prof.py
    DGC_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(dgc::g_es_prof), sizeof(dgc::g_es_prof)));
    return DGC_OK;
}

extern "C" int dgc_pass_prof(void* out) {   // tools/pass_prof.py
    DGC_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(dgc::g_pass_prof), sizeof(dgc::g_pass_prof)));
    return DGC_OK;
}

extern "C" int dgc_rs_prof(void* out) {   // tools/k3_prof.py
    DGC_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(dgc::g_rs_prof), sizeof(dgc::g_rs_prof)));
    return DGC_OK;
}

extern "C" int dgc_k5_prof(void* out, int reset) {
    if (reset) {
        dgc::K5Prof z{};
        DGC_HIP(hipMemcpyToSymbol(HIP_SYMBOL(dgc::g_k5prof), &z, sizeof(z)));
        return DGC_OK;
    }
    DGC_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(dgc::g_k5prof), sizeof(dgc::K5Prof)));
    return DGC_OK;
}
#endif

extern "C" int dgc_compress_flush(float* vec, float* mmt, int64_t sample_stride, const dgc_select_params* params,
                                  void* ws, size_t ws_bytes, void* stream) {
    return dgc::compress_flush(vec, mmt, sample_stride, params, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int dgc_batch_flush(const dgc_batch_desc* batch, float* mmt, float* vec, void* ws, size_t ws_bytes,
                               void* stream) {
    return dgc::batch_flush(batch, mmt, vec, ws, ws_bytes, static_cast<hipStream_t>(stream));
}
