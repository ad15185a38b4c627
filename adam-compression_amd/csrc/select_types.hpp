// Selection, shared types: the segment / list constants and the list-slot helpers
// (lcol, lslot), the device tables (TDesc, SelState, SetG, SelCfg), the block-table ids
// (BT_*), the workspace (SelWS) and nth_cand_cap. Every other select_*.hpp includes it,
// directly or through an earlier stage; it relies on radix_select.hpp (RSState) and
// introselect.hpp (NthG), and through them on dgc_common.hpp (kBlock, kWave).
#pragma once
#include "radix_select.hpp"
#include "introselect.hpp"

namespace dgc {
constexpr int kSeg = 1024;                      // elements per segment
constexpr int kCap = 64;                        // list slots per segment (6.25 %)
// The lists of kLstTile consecutive segments interleave: entry e of segment s sits at
// lcol(s) + e * kLstTile, so a 128-B line holds entries 0..7 of four lists. The
// selection reads a list per segment (~7 entries at 1e-3): contiguous 256-B list slots
// cost a line per segment there, the interleave a line per four. The four segments of
// a tile are K1's (and the select pass's) four waves of one workgroup, so the tile's
// lines fill in one L2.
constexpr int kLstTile = 4;
__host__ __device__ __forceinline__ int64_t lcol(int64_t seg) {
    return (seg / kLstTile) * (kLstTile * kCap) + seg % kLstTile;
}
// Slot of entry e of segment seg: every list access goes through it (DESIGN.md §5 has the
// banded layout that was measured and dropped).
__host__ __device__ __forceinline__ int64_t lslot(int64_t seg, int64_t e) { return lcol(seg) + e * kLstTile; }
constexpr int kSegTiles = kSeg / (kWave * 4);   // 4 float4 per lane per segment
constexpr int kSuper = 4;                       // segments per wave in the full select pass
constexpr int kGroupSegs = 1024;                // segments per group (1M elements)
constexpr int kCountSegs = 4;                   // k_count_lists: segments per thread (a group per block)
constexpr int kSegPerBlock4 = kBlock / kWave;   // 4 waves per workgroup
constexpr int kSegPerBlock16 = kSegPerBlock4 * kSuper;
constexpr int kMaxLower = 16;                   // thresholds per multi-threshold pass
constexpr int kSpillShards = 64;
constexpr int kSpillDiv = 32;                   // lists dropped when > nseg/32 segments spill
constexpr int kQueuePerBlock = kBlock;          // K5 emit: outputs per workgroup
constexpr int kCapBlocks = 2048;                // grid-stride launches: blocks per whole bucket (one tensor)
constexpr int kCapBlocksBatch = 16384;          // ... per whole batch of several tensors
// The adaptive list margin's ceiling (k_sel_finish, spec[4]): kSpecCeil0 at first, up by
// kSpecCeilUp after every hit to kSpecMarginMax, down by kSpecCeilDown after a miss.
constexpr float kSpecCeil0 = 0.95f;
constexpr float kSpecMarginMax = 0.985f;
constexpr float kSpecCeilUp = 0.005f, kSpecCeilDown = 0.05f;
// K5s, the set path of an untied resample (resample_order = 1; see k_resample_set): one
// launch, workgroups per tensor by its candidate capacity (BT_SET) — one up to
// kSetCoopMin, then one per kSetCoopMin candidates, from kSetGDefault to kSetGBig
// (VGG-16-BN's fc6) — kSetRegC rounds of 1024 keys per workgroup in registers (32 spilled
// the radix passes' registers to scratch), up to kSetRoundsMax rounds from L2 beyond.
constexpr int kSetGDefault = 4;                 // a cooperative set's fewest workgroups
constexpr int kSetGBig = 128;
constexpr int kSetRegC = 16;
constexpr int kSetRoundsMax = 64;
constexpr int64_t kSetCoopMin = (int64_t)kSetRegC * 1024;   // (kScanThreads keys per round)
// its radix select: two passes over key - key(t_cur), bits [kSetLo0, kSetSpan) clamped
// (the top bin takes every key past the span) then [0, kSetLo0)
constexpr int kSetSpan = 25, kSetLo0 = 13;
constexpr int kSetBins0 = 1 << (kSetSpan - kSetLo0), kSetBins1 = 1 << kSetLo0;   // 4096, 8192
constexpr int kSpecWords = 8;                   // per-tensor speculation state (dgc_compress_begin: spec)
constexpr int kChainOneWords = 256;             // SelWS::chain: k_chain_one's words (zeroed every call) ...
constexpr int kChainWords = kChainOneWords + 128;   // ... then k_rs_passes' (zero at rest)
constexpr int kEmitSplit = 4;                   // k_emit workgroups per group
constexpr int64_t kSetOneMax = kSetCoopMin;     // K5s: one workgroup up to this many candidates
constexpr int64_t kQueueFold = 16384;           // k_nth_select emits its replay itself when every k <= this

// One compressed tensor (device table, built on the host).
struct TDesc {
    int64_t n;              // numel
    int64_t off;            // element offset in the flat grad / mmt / vec buffers (multiple of kSeg)
    int64_t seg0, nseg;     // global segments
    int64_t grp0, ngrp;     // global groups
    int64_t k, S, ks, stride;          // num_selects, num_samples, top_k_samples, sample_stride
    int64_t upper_count, lower_count;  // floor(k * upper), ceil(lower * k)
    int64_t samp_off;       // offset of its samples in the flat sample buffer; -1: none / N == S
    int64_t win_off, win_cap;          // its K1 sample window list in the sample buffer (cap 0: none)
    int64_t whist_off;                 // K1's histogram of that window (kWinBins u32, zero at rest)
    int64_t cand_off, cand_cap;        // K5 queue region: min(N, 64k - 1) candidates
    int64_t gpos_off;       // K5 pair slots: 2 x (cand_cap / 2 + 1)
    int64_t idx_base;       // added to the emitted indices (its flat offset in a batch, 0 alone)
    int64_t nv4;            // float4s that K1 streams (n/4 unpadded, ceil(n/4) padded)
    double inv_stride;
    float inv_stride_f;
    int32_t tail;           // the elements [4*nv4, n) are compensated outside K1 (unpadded)
};

struct SelState {
    float t0, t_cur, t_list;
    int32_t branch, iter, recounts, active;
    long long n_cur;       // count at t_cur
    long long limit;       // FIRSTK: emit the first `limit` candidates
    int32_t overflow, done, lower_pending;
    int32_t full_passes, list_spills, epoch;
    int32_t rs_nth;        // RESAMPLE: 1 = nth_element replay (K5), 2 = partial_sort replay (K5b)
    int32_t tie_rule;      // DGC_TIES_*: how the resample chose among boundary ties
    // Deferred momentum masking (DGCSGDMemory.update, dgc/memory.py:72-77): the last
    // call emitted "the first def_limit elements >= def_t" without zeroing them; the
    // next K1, which streams vec and mmt anyway, zeroes them before compensating.
    int32_t def_mode, def_mask_mmt;
    float def_t;
    int32_t win_keys;      // keys K3 read from the K1 sample window list (0: the samples)
    uint32_t win_key;      // the window's key (K1's block 0): its histogram's bin 0
    long long def_limit;
    uint32_t tickets[4];
    uint32_t tk8[9];       // sharded arrival of the count passes (last_block_arrival8)
    uint32_t ce_ticket;    // k_count_emit: groups in ticket order (look-back)
    int32_t ce_fail;       // k_count_emit: a look-back timed out (its emit is not trusted)
    int32_t spec_emitted;  // k_count_emit's first-k payload stands: k_emit skips the tensor
    // Segments whose K1 list overflowed, counted by K1 into slot [epoch & 1] (64
    // shards against atomic contention); k_sel_init reads it and zeroes the other
    // slot for the next call, k_sel_finish advances the epoch.
    uint32_t spill[2][kSpillShards];
    // Samples with key >= key(t_list) that K1 appended to the tensor's window list, in
    // slot [epoch & 1] like spill (the count runs past win_cap when the list overflows).
    uint32_t win_cnt[2];
    unsigned long long lower_cnt[kMaxLower + 1];   // counts at t_1..t_m (multi-threshold pass)
};

// K5s over co-resident workgroups per tensor (k_resample_set): the residency consensus,
// the barrier, the key range and the per-pass histograms. arrive / decide / bar_* /
// broken / mn / mx are reset by sel_init_tensor every call; hist is zero at rest (the
// workspace is zero-filled at init; the workgroups re-zero what they used).
struct SetG {
    uint32_t arrive, decide, bar_count, bar_gen, broken;
    uint32_t gathered;                      // k_emit_set: the tensor's emit workgroups done with its gather
    uint32_t mn, mx;
    uint32_t cnt[kSetGBig];                 // per workgroup: its candidates >= the k-th key
    uint32_t hist0[kSetBins0], hist1[kSetBins1];   // the radix passes' merged histograms
};

// Per-call settings shared by the tensors.
struct SelCfg {
    float upper, lower;         // fl32(compress_upper_bound), fl32(compress_lower_bound)
    int32_t max_iters, resample, masking, vdtype, idtype;
    int32_t update_memory;      // 0: none, 1: zero the emitted slots now, 2: deferred to the next K1
    int32_t tdtype;             // the sparsified tensor's dtype: threshold *= bound rounds to it
    int32_t set_order;          // resample_order = 1: an untied resample emits its set in index order (K5s)
};

// Block tables: prefix arrays [T + 1] of per-tensor workgroup counts for one launch shape.
enum { BT_K1 = 0, BT_FULL, BT_CAP16, BT_CAP4, BT_FULL8, BT_CAP8, BT_SEG, BT_GRP, BT_QUEUE, BT_SAMP, BT_CNT, BT_SET, BT_COUNT };

struct SelWS {
    int32_t T;
    TDesc* td;
    SelState* st;
    RSState* rs;               // [T]: K3 thresholds, then the resample's radix select
    float* thr;                // [T] sampled thresholds
    float* spec;               // [2T] speculative list thresholds (null: none), persistent
    int64_t* starts;           // [T] sample starts of this call
    const float** gptr;        // [T] per-tensor gradient pointers of this call (K1 from a pointer table)
    int64_t* scnt;             // [T] strided sample counts of this call
    float* samples;            // flat sample buffer
    int32_t* bt[BT_COUNT];     // block tables
    int32_t* small;            // tensors whose threshold runs in one workgroup
    uint32_t* seg_lcnt;        // list count at t_list (low 16 bits) | lmax_code (high 16 bits)
    uint32_t* seg_cnt;
    uint32_t* seg_off;         // in-group output offset of each segment's first emitted entry
    uint16_t* lst_off;
    float* lst_val;
    unsigned long long* grp_cnt;
    long long* grp_off;
    unsigned long long* grp_lb;    // k_count_emit's decoupled look-back words, one per group
    uint64_t* queue;           // K5: (|x| key << 32 | j) for the candidates j, ascending index order
    int64_t* cand_idx;         // K5: the candidates' element indices (within the tensor)
    float* cand_val;           // K5: their values (what the gather read; the set path's emit)
    uint32_t* cand_key;        // K5: their |x| keys, dense (the set paths read 4 B per candidate, not 8)
    uint32_t* gpos;            // K5: pair slots of the global-memory partition passes
    NthG* nthg;                // [T] K5: the multi-workgroup global phase's state
    SetG* setg;                // [T] K5s over a set's workgroups of one launch
    uint32_t* fin_ticket;      // k_nth_select's last-workgroup ticket (zeroed by sel_init_tensor)
    uint32_t* chain;           // k_chain_one's claim / completion / gate words (zeroed by sel_init_tensor)
    int64_t nseg, ngrp;
};

// Candidates the nth_element replay (K5) gathers: torch's CPU topk runs nth_element
// while k * 64 > n (else partial_sort, replayed over vec by K5b), so at most 64k - 1.
__host__ __device__ inline int64_t nth_cand_cap(int64_t numel, int64_t k) {
    const int64_t c = 64 * k - 1;
    return c < numel ? c : numel;
}
}  // namespace dgc
