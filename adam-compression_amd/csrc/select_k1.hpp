// Selection, K1: compensate + strided sample + the speculative candidate lists
// (k_compensate_list, over fp32 state and an fp32 or a 16-bit gradient; k_compensate_tail_g16,
// the scalar tail of the latter), and k_no_lists for a call whose vec no K1 listed. Relies on
// select_layout.hpp (OneTable, StartChunk) and select_tiles.hpp (loads, list_append,
// the deferred masking).
#pragma once
#include "select_tiles.hpp"

namespace dgc {
// ---- The 8-B streaming access to four 16-bit elements per lane: K1's 16-bit gradient and
// all of K1-16 (select_k1_16.hpp).
typedef uint32_t u2v __attribute__((ext_vector_type(2)));

// (uint2 in registers, like ld_nt's float4: an array of ext vectors is merged into one
// wide value, and every conditional load of a part then copies — and waits for — the whole)
__device__ __forceinline__ uint2 ld_nt(DGC_GLB const u2v* p) {
    const u2v x = __builtin_nontemporal_load(p);
    return make_uint2(x[0], x[1]);
}
__device__ __forceinline__ void st_nt(DGC_GLB u2v* p, uint2 v) {
    const u2v x = {v.x, v.y};
    __builtin_nontemporal_store(x, p);
}

template <int DT>
__device__ __forceinline__ void unpack4(uint2 q, float (&x)[4]) {
    x[0] = h16_to_f32<DT>((uint16_t)(q.x & 0xFFFFu));
    x[1] = h16_to_f32<DT>((uint16_t)(q.x >> 16));
    x[2] = h16_to_f32<DT>((uint16_t)(q.y & 0xFFFFu));
    x[3] = h16_to_f32<DT>((uint16_t)(q.y >> 16));
}

// K1's gradient by dtype GD: the element the kernel's pointer names, a lane's streaming
// load of four of them, and that load in registers.
template <int GD> struct K1Grad { typedef uint16_t elem; typedef u2v load; typedef uint2 reg; };
template <> struct K1Grad<DGC_F32> { typedef float elem; typedef float4 load; typedef float4 reg; };

// task() that also returns the tensor's first block, blk[t], from the words the search
// has loaded: the largest entry <= b of the ascending table (blk[0] = 0). K1 would
// otherwise read it back, one more round trip ahead of its streaming loads.
__device__ __forceinline__ int task_first(const int32_t* blk, int T, int b, int64_t& b0) {
    b0 = 0;
    if (T <= 1) return 0;
    const int lane = threadIdx.x & 63;
    int cnt = 0;
    uint32_t first = 0;
    for (int i0 = 0; i0 < T; i0 += 64) {
        const int i = i0 + lane;
        const int32_t v = i < T ? blk[i] : 0x7FFFFFFF;
        const bool le = v <= b;
        const uint64_t m = __ballot(le);
        cnt += __popcll(m);
        first = max(first, le ? (uint32_t)v : 0u);
        if (m != ~0ull) break;   // ascending table: every later entry is > b
    }
    b0 = wave_max(first);
    return __builtin_amdgcn_readfirstlane(cnt - 1);
}

// ---- The steps K1 and K1-16 (select_k1_16.hpp) share from the moment a tile's new velocity
// x[4] stands in registers. A one-tensor call's table stores (w.td[0] = ot.d, ...) are not
// among them: in a helper (SelWS and OneTable by value) they cost the one-tensor kernels
// registers and a wave per SIMD (DESIGN.md §5 "K1's shared steps"; tools/k1_isa.py shows it).

// Their wave-uniform set-up, once everything a wave loads is in flight. The call's first
// thread publishes t_list, the window's key and (put_start) the sample start and count.
struct K1Seg {
    float tl;            // list threshold spec[0] (inf: no lists)
    // the sample window: every sample with key >= win_key, inf and NaN too. Its threshold
    // spec[2] predicts this call's sampled threshold from just below; before the first
    // prediction it is the list threshold
    uint32_t win_key;
    bool windowed;
    float *sout, *win;
    uint32_t *win_cnt, *whist;
    int64_t scount, q0, r0;   // samples; floor divmod of (the segment's first element - start) by the stride
};
__device__ __forceinline__ K1Seg k1_segment_begin(const SelWS& w, const TDesc& d, int t, DGC_GLB SelState* st,
                                                  bool first, bool put_start, float spec0, float spec2,
                                                  int32_t epoch, int64_t ls, int64_t start, int64_t scount) {
    const bool sample = d.samp_off >= 0;
    K1Seg k;
    k.tl = w.spec ? spec0 : __builtin_huge_valf();
    if (first) st->t_list = k.tl;
    if (put_start && first) {
        w.starts[t] = start;
        w.scnt[t] = sample ? scount : d.n;
    }
    k.sout = sample ? w.samples + d.samp_off : nullptr;
    k.win = w.samples + d.win_off;
    const float tw = w.spec ? spec2 : __builtin_huge_valf();
    k.win_key = abs_key(tw < __builtin_huge_valf() ? tw : k.tl);
    k.windowed = sample && d.win_cap > 0;
    k.win_cnt = &w.st[t].win_cnt[epoch & 1];
    k.whist = reinterpret_cast<uint32_t*>(w.samples + d.whist_off);
    if (k.windowed && first) st->win_key = k.win_key;
    k.scount = scount;
    k.q0 = k.r0 = 0;
    if (sample) floor_divmod_fast(ls * kSeg - start, d.stride, d.inv_stride, k.q0, k.r0);
    return k;
}

// The per-tile sample of a sampled tensor. A lane's group gi (= 64 * u + lane) holds at most
// one sample (stride >= 4): its element j, the tensor's sample qi. Writes |x[j]| to
// sout[qi]; returns whether it joins the window (window: this group may), hv its value.
__device__ __forceinline__ bool k1_sample(const K1Seg& k, const TDesc& d, const float (&x)[4], uint32_t valid,
                                          int gi, bool window, float& hv) {
    const uint32_t s32 = (uint32_t)d.stride;
    uint32_t q1, r;
    divmod_u32((uint32_t)k.r0 + 4u * (uint32_t)gi, s32, d.inv_stride_f, q1, r);
    const uint32_t j = r == 0 ? 0u : s32 - r;
    if (j >= 4 || !((valid >> j) & 1u)) return false;
    const int64_t qi = k.q0 + q1 + (r == 0 ? 0 : 1);
    if (qi < 0 || qi >= k.scount) return false;
    hv = fabsf(x[j]);
    k.sout[qi] = hv;
    return window && __float_as_uint(hv) >= k.win_key;
}

// The window append of a tile's hits: wave-uniform and rare (~3 ks of the S samples), one
// atomic on the count per wave; the count runs past win_cap when the list overflows.
__device__ __forceinline__ void k1_window_append(const K1Seg& k, int64_t win_cap, bool hit, float hv, int lane) {
    const uint64_t hb = __ballot(hit);
    if (!hb) return;
    const int leader = __ffsll((unsigned long long)hb) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(k.win_cnt, (uint32_t)__popcll(hb));
    base = __shfl(base, leader);
    const uint32_t pos = base + (uint32_t)__popcll(hb & ((1ull << lane) - 1));
    if (hit && pos < (uint64_t)win_cap) k.win[pos] = hv;
    if (hit) atomicAdd(&k.whist[win_bin(__float_as_uint(hv), k.win_key)], 1u);   // (no return value)
}

// The segment end: its exact count at t_list with the code of its largest key, or the
// spilled mark of the segment with a scalar tail; one atomic per wave with a spilled segment
// (c is wave-uniform) into spill, the tensor's shards of this epoch, sharded by block.
__device__ __forceinline__ void k1_segment_end(uint32_t c, uint32_t mk, bool put, bool tail, uint32_t* seg_lcnt,
                                               uint32_t* spill) {
    mk = wave_max(mk);
    if (!put) return;
    *seg_lcnt = tail ? lcnt_pack(kCap + 1, 0xFFFFu) : lcnt_pack(c, lmax_code(mk));
    if (c > (uint32_t)kCap) atomicAdd(&spill[blockIdx.x % kSpillShards], 1u);
}

// K1 (compensate + strided sample, see compensate.hip) that also lists every
// element with |vec_new| >= t_list into its segment's list. One wave per segment:
// float4 index = 256*seg + 64*u + lane (u = 0..3), each instruction 1 KB contiguous;
// non-temporal loads and stores. seg_lcnt = exact count at t_list; a segment that
// holds an unpadded scalar tail is marked spilled (re-read when needed).
// ONE (a one-tensor call): the tensor's tables ride in the arguments (ot) — block 0
// writes them into the workspace for the kernels after K1, which replaces a k_put_one
// launch before every K1 (and its wait) — and the sample start in sc.
// CLIP: the gradient clipped as it is used (dgc_common.hpp clip1), tensor t's
// coefficient from ca; DGC_CLIP_NONE compiles to the unclipped kernel.
// GD: the gradient's dtype. DGC_BF16 / DGC_F16 is the flat bucket's 16-bit gradient onto fp32
// state (dgc_compress_begin_g16), one-tensor and unclipped: the reference's compensate there
// (dgc/memory.py:50-63) runs every op in fp32 on the exactly widened gradient (torch's type
// promotion of the in-place ops), so the step is bit for bit the fp32 one on grad.float().
// The gradient is then an 8-B load per lane (512 B per instruction) widened by unpack4, with
// the fp32 kernel's lane-to-element mapping: 18 B/elem where grad.float() and the fp32 kernel
// move 6 + 20, and 10 KB in flight per wave. It is exactly n elements and the state is unpadded
// (d.nv4 = n / 4 full groups): a live lane loads group gi of all three arrays only while
// gi < n / 4, so the last byte read is below element 4 * (n / 4) <= n of each. The n & 3
// elements after it are k_compensate_tail_g16's; their samples are read back from vec and
// their segment is marked spilled (d.tail), as dgc_compress_begin does.
// One template, not a sibling kernel: the parameter renames the fp32 instantiations and leaves
// their code as it was, instruction for instruction (tools/kernel_hashes.py --diff reports
// all twelve as renamed), and the 16-bit ones keep the sibling's registers and occupancy.
//
// The order of a wave's memory reads is the kernel's schedule (DESIGN.md §5 "K1's
// schedule", tools/k1_isa.py): every state word it will need (the speculation thresholds,
// the SelState fields, the deferred masking's offsets, a large batch's table entries) is
// an independent load of a wave-uniform address ahead of any store of the kernel, so a
// scalar load on its own counter, and its twelve 16-B streaming loads go out through
// global-typed pointers before the first use of either kind (the compiler places the
// scalar loads right behind the streaming ones). A one-tensor wave so waits for nothing
// but its arguments until 12 KB are in flight. How many such waves a CU holds is the
// launch's business (select.hip, kK1FlatLds).
//
// A null spec or clip table is replaced by the tensor's own state as "any readable words":
// the kernel then reads words 0 and 2 of SelState and ignores them.
static_assert(offsetof(SelState, t0) == 0 && offsetof(SelState, t_list) == 2 * sizeof(float),
              "K1's stand-in for a null spec reads SelState words 0 and 2");
template <bool NEST, bool ONE, int CLIP, int GD = DGC_F32>
__global__ void __launch_bounds__(kBlock)
k_compensate_list(const typename K1Grad<GD>::elem* __restrict__ g_flat, float* __restrict__ mmt_flat,
                  float* __restrict__ vec_flat, float mom, SelWS w, StartChunk sc, int wt, OneTable ot, ClipArg ca) {
    // (the reference clips a 16-bit gradient in its own dtype, clip16, which this kernel does not)
    static_assert(GD == DGC_F32 || (ONE && CLIP == DGC_CLIP_NONE), "a 16-bit gradient: one tensor, unclipped");
    int64_t b0 = 0;   // the tensor's first block
    const int t = ONE ? 0 : task_first(w.bt[BT_K1], w.T, blockIdx.x, b0);
    const TDesc d = ONE ? ot.d : w.td[t];   // by value: stores below cannot alias it
    const int lane = threadIdx.x & 63, wave = wave_id();
    const int64_t ls = ((int64_t)blockIdx.x - b0) * kSegPerBlock4 + wave;   // local segment
    // a wave past the tensor's last segment loads nothing and lists nothing (no early
    // exit: a branch here would split the table reads into two round trips)
    const bool live = ls < d.nseg;
    const bool first = blockIdx.x == b0 && threadIdx.x == 0;
    // sample starts (and gradient pointers) of the first sc.count tensors ride in the arguments
    const bool arg_start = ONE || t < sc.count;
    const bool ptrs = !ONE && sc.ptrs;   // a one-tensor call reads the flat gradient
    const bool sample = d.samp_off >= 0;

    // ---- the state words, one batch (uses further down)
    DGC_GLB SelState* st = glb(w.st + t);
    DGC_GLB const float* spec = w.spec ? glb(w.spec + kSpecWords * t) : &st->t0;   // (null: any readable words)
    const float spec0 = spec[0], spec2 = spec[2];
    const int32_t epoch = st->epoch, def_mode = st->def_mode, def_mask_mmt = st->def_mask_mmt;
    const float def_t = st->def_t;
    const long long def_limit = st->def_limit;
    // the deferred masking's offsets: the slots exist for ls < d.nseg whether or not a
    // masking is pending. A one-tensor call has their addresses from its arguments; a
    // batch has them from td[t], which its streaming loads wait for too, so there they
    // go out right behind the streaming loads instead of one round trip ahead of them
    const int64_t lsd = live ? ls : 0;
    DGC_GLB const long long* grp_off = glb(w.grp_off) + (d.grp0 + lsd / kGroupSegs);
    DGC_GLB const uint32_t* seg_off = glb(w.seg_off) + (d.seg0 + lsd);
    long long def_rank = 0;
    if (ONE) def_rank = *grp_off + (long long)*seg_off;
    float cf_tab = 0.f;
    if (CLIP != DGC_CLIP_NONE) cf_tab = *(ca.tab ? glb(ca.tab + t) : (DGC_GLB const float*)&st->t0);
    int64_t start_ws = 0, scnt_ws = 0;
    const float* gptr_ws = nullptr;
    if (!arg_start) {   // a batch past 64 tensors: k_put_starts wrote them
        start_ws = glb(w.starts)[t];
        scnt_ws = glb(w.scnt)[t];
        if (ptrs) gptr_ws = glb(w.gptr)[t];
    }

    // ---- the streaming loads: momentum and velocity, then the gradient (its pointer may
    // be one of the words above)
    const int64_t n = d.n;
    const int64_t seg4 = ls * (kSeg / 4);
    const int left = (int)min(d.nv4 - seg4, (int64_t)(kSeg / 4));   // float4s of the segment
    // a pointer-table gradient is exactly n floats: its full float4s only
    const int gleft = ptrs ? (int)min((n >> 2) - seg4, (int64_t)(kSeg / 4)) : left;
    DGC_GLB float4* mmt = glb(reinterpret_cast<float4*>(mmt_flat + d.off) + seg4);
    DGC_GLB float4* vec = glb(reinterpret_cast<float4*>(vec_flat + d.off) + seg4);
    const typename K1Grad<GD>::elem* gsrc;
    if constexpr (GD == DGC_F32) gsrc = !ptrs ? g_flat + d.off : (arg_start ? sc.grad[ONE ? 0 : t] : gptr_ws);
    else gsrc = g_flat + d.off;   // flat, exactly n elements: its full groups only (gleft = left)
    DGC_GLB const typename K1Grad<GD>::load* g = glb(reinterpret_cast<const typename K1Grad<GD>::load*>(gsrc) + seg4);
    typename K1Grad<GD>::reg gv[kSegTiles];
    float4 mv[kSegTiles], vv[kSegTiles];
#pragma unroll
    for (int u = 0; u < kSegTiles; ++u) {
        if (u * 64 + lane < left) {
            mv[u] = ld_nt(mmt + u * 64 + lane);
            vv[u] = ld_nt(vec + u * 64 + lane);
        }
    }
#pragma unroll
    for (int u = 0; u < kSegTiles; ++u)
        if (u * 64 + lane < gleft) gv[u] = ld_nt(g + u * 64 + lane);
    // the one wave that owns the partial last float4 of a pointer-table gradient patches
    // it in (wave-uniform branch, one lane loads)
    if constexpr (GD == DGC_F32) {
        if (ptrs && gleft < left && gleft >= 0) {
#pragma unroll
            for (int u = 0; u < kSegTiles; ++u)
                if (u * 64 + lane == gleft) gv[u] = ld_tail4(glb(gsrc), n);
        }
    }

    if (!ONE) def_rank = *grp_off + (long long)*seg_off;

    // ---- everything loaded is in flight: the stores of the call's tables
    if (ONE && first) {
        w.td[0] = ot.d;
        for (int which = 0; which < BT_COUNT; ++which) {
            w.bt[which][0] = ot.bt[which][0];
            w.bt[which][1] = ot.bt[which][1];
        }
        w.small[0] = 0;
    }
    const float cf = ca.tab ? cf_tab : ca.value;
    const int64_t start = !sample ? 0 : (arg_start ? sc.start[ONE ? 0 : t] : start_ws);
    const int64_t scount = !sample ? 0 : (arg_start ? ceil_div(d.n - start, d.stride) : scnt_ws);
    const K1Seg k = k1_segment_begin(w, d, t, st, first, arg_start, spec0, spec2, epoch, ls, start, scount);
    uint32_t c = 0, mk = 0;
    const int64_t seg = d.seg0 + ls;
    if (def_mode && live) apply_deferred_mask(def_t, def_limit, def_mask_mmt != 0, def_rank, d, ls, lane, vv, mv);
#pragma unroll
    for (int u = 0; u < kSegTiles; ++u) {
        const bool ok = u * 64 + lane < left;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        uint32_t valid = 0;
        bool hit = false;   // this lane's sample (at most one per float4: stride >= 4) joins the window
        float hv = 0.f;
        if (ok) {
            // (the four lines twice: fed from one float4 filled under the `if constexpr`, the
            // fp32 kernels came out with two instructions per tile in another order)
            if constexpr (GD == DGC_F32) {
                const float4 gq = clip4<CLIP>(gv[u], cf);
                x[0] = comp1<NEST, true>(gq.x, mv[u].x, vv[u].x, mom);
                x[1] = comp1<NEST, true>(gq.y, mv[u].y, vv[u].y, mom);
                x[2] = comp1<NEST, true>(gq.z, mv[u].z, vv[u].z, mom);
                x[3] = comp1<NEST, true>(gq.w, mv[u].w, vv[u].w, mom);
            } else {
                float gx[4];
                unpack4<GD>(gv[u], gx);   // exact: the reference's promotion of the 16-bit gradient
                x[0] = comp1<NEST, true>(gx[0], mv[u].x, vv[u].x, mom);
                x[1] = comp1<NEST, true>(gx[1], mv[u].y, vv[u].y, mom);
                x[2] = comp1<NEST, true>(gx[2], mv[u].z, vv[u].z, mom);
                x[3] = comp1<NEST, true>(gx[3], mv[u].w, vv[u].w, mom);
            }
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
    // (the segment with the scalar tail, compensated outside K1, is marked spilled)
    k1_segment_end(c, mk, lane == 0 && live, d.tail && ls == d.nseg - 1, w.seg_lcnt + seg, w.st[t].spill[epoch & 1]);
}

// The n & 3 elements [begin, n) after the last full group of a 16-bit gradient: comp1 on the
// widened gradient, one thread each (k_compensate1's arithmetic, compensate.hip, with the
// 16-bit read).
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

__global__ void k_no_lists(SelWS w) {
    for (int t = threadIdx.x; t < w.T; t += blockDim.x) w.st[t].t_list = __builtin_huge_valf();
}
}  // namespace dgc
