// Selection, K5b: torch's partial_sort replayed over vec (heap_select_wg: heap select +
// sort_heap + emit), run by k_nth_select (select_nth.hpp), whose LDS area it shares
// (kK5SmemBytes). Relies on select_emit.hpp (EmitOut, out_base, emit_one) and
// introselect.hpp (kNthThreads, kNthSmemBytes).
#pragma once
#include "select_emit.hpp"

namespace dgc {
// K5b: torch's CPU topk on its partial_sort path (k * 64 <= candidates, i.e. a sampled
// threshold >= 64x too low), replayed EXACTLY for every k and N (dgc/compression.py:
// 134-137): std::partial_sort(queue, queue + k, queue + n, greater) over the
// candidates in index order = make_heap of the first k, then every later candidate
// whose key beats the heap's top replaces it (pop_heap), then sort_heap; queue[0..k)
// is the output in that order. Equal keys are indistinguishable to the heap's
// comparisons, so which boundary ties survive and the order of equal keys come from
// its exact layout — the replay runs the same operations on the same layout.
//
//   entries   (|x| key (31 bits) << 33) | element index (33 bits) for N < 2^33; above, the
//             low 33 bits hold a SLOT in [0, k) and the tensor's cand_idx region maps slot ->
//             element index: the heap holds k entries at any time, and an entry that
//             replaces the root takes the root's slot (its key alone is compared, so the
//             replay is the same)
//   layout    node i in LDS for i < kHeapTop (levels 0..13), else in the tensor's K5
//             queue region (>= k entries: cand_cap = min(64k - 1, N) >= k)
//   fill      the workgroup streams vec in index order, block-scans the candidates
//             (|x| >= t_cur) and writes the first k to nodes 0..k-1
//   make_heap level by level, one thread per parent (parents of one level own
//             disjoint subtrees, so this is std::__make_heap's descending order)
//   select    per 2048-element chunk, the candidates that beat the root are compacted
//             in order; wave 0 re-checks each against the live root and replaces it:
//             the min-child path to a leaf is found 5 levels per load (62 lanes load
//             the hole's subtree, the path is resolved with readlanes), then
//             std::__push_heap's stop on the (monotone) path is one ballot, and the
//             shifted nodes are written in parallel
//   sort_heap k - 1 pops by wave 0, the same replacement on a shrinking heap
//   emit      payload slot p <- node p: values, wire casts, DGCSGDMemory.update's masking
//
// Sequential by nature (~k ln(n/k) replacements + k pops); reached only when the
// sampled threshold came out >= 64x too low, never by the benchmarked workloads.
constexpr int kHeapTop = 16383;                  // nodes in LDS (levels 0..13)
constexpr int kHeapChunk = kNthThreads * 4;      // vec elements per step: one float4 per thread
constexpr int kHeapSub = 5;                      // levels of the path resolved per load
constexpr int kHeapKeyShift = 33;
constexpr uint64_t kHeapIdxMask = (1ull << kHeapKeyShift) - 1;
constexpr size_t kHeapSmemBytes = (size_t)(kHeapTop + 1 + kHeapChunk) * 8;   // nodes + hot list
constexpr size_t kK5SmemBytes = kHeapSmemBytes > kNthSmemBytes ? kHeapSmemBytes : kNthSmemBytes;

__device__ __forceinline__ uint32_t hkey(uint64_t e) { return (uint32_t)(e >> kHeapKeyShift); }

struct HeapNodes {
    DGC_LDS uint64_t* l;   // nodes [0, kHeapTop)
    DGC_GLB uint64_t* g;   // nodes >= kHeapTop (indexed by node)
    __device__ __forceinline__ uint64_t ld(int64_t i) const { return i < kHeapTop ? l[i] : g[i]; }
    __device__ __forceinline__ void st(int64_t i, uint64_t v) const {
        if (i < kHeapTop)
            l[i] = v;
        else
            g[i] = v;
    }
};

// std::__adjust_heap + std::__push_heap on nodes [0, len) from `hole` with value v,
// comp = key greater (the root holds the smallest key). One thread (make_heap).
__device__ void heap_adjust1(const HeapNodes& h, int64_t hole, int64_t len, uint64_t v) {
    const int64_t top = hole;
    int64_t child = hole;
    while (child < (len - 1) / 2) {
        child = 2 * (child + 1);
        const uint64_t r = h.ld(child), l = h.ld(child - 1);
        uint64_t c = r;
        if (hkey(r) > hkey(l)) {
            child--;
            c = l;
        }
        h.st(hole, c);
        hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) {
        child = 2 * (child + 1);
        h.st(hole, h.ld(child - 1));
        hole = child - 1;
    }
    int64_t parent = (hole - 1) / 2;
    while (hole > top) {
        const uint64_t pv = h.ld(parent);
        if (!(hkey(pv) > hkey(v))) break;
        h.st(hole, pv);
        hole = parent;
        parent = (hole - 1) / 2;
    }
    h.st(hole, v);
}

__device__ __forceinline__ uint64_t readlane64(uint64_t x, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}

// std::__adjust_heap(first, 0, len, v) — the root replaced by v — by ONE wave (all 64
// lanes, uniform arguments). Returns the new root. The min-child path from the root:
// lanes 2^d - 2 .. 2^(d+1) - 3 hold the hole's descendants at depth d = 1..5, loaded
// at once; the choice at each level (right child unless the left key is smaller;
// a lone left child at the end) is resolved from them with readlanes. Along the path
// the keys never decrease (heap order), so push_heap's climb stops at J = the first
// path node whose key exceeds v's: nodes p_0..p_(J-2) take the values of p_1..p_(J-1),
// p_(J-1) takes v, the rest keep theirs — written by lanes 0..J-1 at once.
__device__ uint64_t heap_replace_root(const HeapNodes& h, int64_t len, uint64_t v) {
    const int lane = threadIdx.x & 63;
    uint64_t pidx = 0, pval = 0;   // lane j-1: path node p_j and its value a_j
    int m = 0;                     // path length
    int64_t hole = 0;
    bool more = len > 1;
    while (more) {
        // this lane's descendant of `hole`: depth dl (1..5), offset ol
        const int dl = 31 - __clz(lane + 2);               // lane + 2 in [2^dl, 2^(dl+1))
        const int64_t ol = (int64_t)(lane + 2) - (1ll << dl);
        const int64_t node = ((hole + 1) << dl) - 1 + ol;
        uint64_t val = 0;
        if (lane < 62 && node < len) val = h.ld(node);
        int64_t off = 0;   // the hole's offset among the subtree nodes of its depth
        for (int d = 1; d <= kHeapSub; ++d) {
            const int base = (1 << d) - 2;
            int64_t child;
            uint64_t cval;
            if (hole < (len - 1) / 2) {   // two children
                const uint64_t l = readlane64(val, base + (int)(2 * off));
                const uint64_t r = readlane64(val, base + (int)(2 * off) + 1);
                if (hkey(r) > hkey(l)) {
                    child = 2 * hole + 1;
                    cval = l;
                    off = 2 * off;
                } else {
                    child = 2 * hole + 2;
                    cval = r;
                    off = 2 * off + 1;
                }
            } else if ((len & 1) == 0 && hole == (len - 2) / 2) {   // a lone left child, then stop
                child = 2 * hole + 1;
                cval = readlane64(val, base + (int)(2 * off));
                off = 2 * off;
                more = false;
            } else {
                more = false;
                break;
            }
            if (lane == m) {
                pidx = (uint64_t)child;
                pval = cval;
            }
            ++m;
            hole = child;
            if (!more) break;
        }
    }
    // J - 1 = the first lane (path index) whose value's key exceeds v's; m if none
    const uint64_t above = __ballot(lane < m && hkey(pval) > hkey(v));
    const int jm1 = above ? __builtin_ctzll(above) : m;
    const uint64_t up = (uint64_t)__shfl_up((long long)pidx, 1);
    const int64_t parent = lane == 0 ? 0 : (int64_t)up;   // p_(lane) for lane >= 1, p_0 = root
    if (lane < jm1)
        h.st(parent, pval);   // p_(lane) <- a_(lane+1)
    else if (lane == jm1)
        h.st(parent, v);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // the next replacement reads these
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    return jm1 == 0 ? v : readlane64(pval, 0);
}

// Chunk loads: 4 consecutive elements of vec per thread, kHeapAhead chunks (16 KB) in
// flight per batch, the next batch issued before the current one is processed — the
// workgroup streams vec at a CU's load rate instead of one round trip per chunk.
constexpr int kHeapAhead = 8;

__device__ __forceinline__ void heap_load(const float* vec, int64_t n, int64_t c0, bool al, float (&x)[4]) {
    const int64_t e0 = c0 + 4 * (int64_t)threadIdx.x;
    if (al && e0 + 3 < n) {
        const float4 v = *reinterpret_cast<const float4*>(vec + e0);
        x[0] = v.x;
        x[1] = v.y;
        x[2] = v.z;
        x[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = e0 + j < n ? vec[e0 + j] : 0.f;
    }
}

// Candidate bits of a thread's 4 elements at chunk c0 (|x| >= tc; NaN never is).
__device__ __forceinline__ uint32_t heap_cands(int64_t n, int64_t c0, float tc, const float (&x)[4]) {
    const int64_t e0 = c0 + 4 * (int64_t)threadIdx.x;
    uint32_t cm = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) cm |= (uint32_t)(e0 + j < n && fabsf(x[j]) >= tc) << j;
    return cm;
}

// Streams the chunks from c_begin in index order, kHeapAhead at a time with the next
// batch in flight; f(c0, x) returns false to stop (uniformly). Returns the chunk it
// stopped at (n rounded up to a chunk when it ran to the end).
template <class F>
__device__ __forceinline__ int64_t heap_stream(const float* vec, int64_t n, int64_t c_begin, bool al, F&& f) {
    constexpr int64_t kBatch = (int64_t)kHeapAhead * kHeapChunk;
    float xa[kHeapAhead][4], xb[kHeapAhead][4];
#pragma unroll
    for (int u = 0; u < kHeapAhead; ++u) heap_load(vec, n, c_begin + u * kHeapChunk, al, xa[u]);
    for (int64_t b0 = c_begin; b0 < n; b0 += kBatch) {
#pragma unroll
        for (int u = 0; u < kHeapAhead; ++u) heap_load(vec, n, b0 + kBatch + u * kHeapChunk, al, xb[u]);
#pragma unroll
        for (int u = 0; u < kHeapAhead; ++u) {
            const int64_t c0 = b0 + u * kHeapChunk;
            if (c0 >= n) return c0;
            if (!f(c0, xa[u])) return c0;
        }
#pragma unroll
        for (int u = 0; u < kHeapAhead; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) xa[u][j] = xb[u][j];
    }
    return n;
}

__device__ __forceinline__ void heap_select_wg(const float* __restrict__ vec_flat, const SelWS& w, const EmitOut& o, int t,
                               uint64_t* smem) {
    const SelState* st = w.st + t;
    const TDesc d = w.td[t];   // by value: stores below cannot alias it
    const float* vec = vec_flat + d.off;
    const float tc = st->t_cur;
    const int64_t k = d.k, n = d.n;
    const bool al = aligned16(vec);
    const HeapNodes h{lds(smem), glb(w.queue + d.cand_off)};
    // wide (N >= 2^33): node payloads are slots, side[slot] the element index
    const bool wide = n >= ((int64_t)1 << kHeapKeyShift);
    DGC_GLB int64_t* side = glb(w.cand_idx + d.cand_off);
    uint64_t* hot = smem + kHeapTop + 1;
    __shared__ uint64_t lds16[16];
    __shared__ uint64_t root_sh;
    __shared__ long long obase_s;
    const int tid = threadIdx.x;
    // ---- fill: the first k candidates, in index order, become nodes 0..k-1
    int64_t filled = 0, skip = 0;   // skip: candidates of the last fill chunk that went into the heap
    const int64_t c_fill = heap_stream(vec, n, 0, al, [&](int64_t c0, const float (&x)[4]) -> bool {
        const uint32_t cm = heap_cands(n, c0, tc, x);
        uint64_t total;
        uint64_t r = block_exclusive_scan((uint64_t)__popc(cm), lds16, &total);
        const int64_t e0 = c0 + 4 * (int64_t)tid;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if ((cm >> j) & 1u) {
                const int64_t g = filled + (int64_t)r++;
                if (g < k) {
                    h.st(g, ((uint64_t)abs_key(x[j]) << kHeapKeyShift) | (uint64_t)(wide ? g : e0 + j));
                    if (wide) side[g] = e0 + j;
                }
            }
        }
        if (filled + (int64_t)total >= k) {
            skip = k - filled;
            filled = k;
            return false;
        }
        filled += (int64_t)total;
        return true;
    });
    __syncthreads();
    // ---- make_heap, level by level (deepest parents first)
    if (k >= 2) {
        const int64_t last_parent = (k - 2) / 2;
        const int top_level = 63 - __clzll((unsigned long long)(last_parent + 1));
        for (int lv = top_level; lv >= 0; --lv) {
            const int64_t p0 = (1ll << lv) - 1;
            const int64_t p1 = std::min<int64_t>((2ll << lv) - 2, last_parent);
            for (int64_t p = p0 + tid; p <= p1; p += kNthThreads) heap_adjust1(h, p, k, h.ld(p));
            __syncthreads();
        }
    }
    // ---- heap select over the candidates after the first k, from the chunk the fill ended in
    if (tid == 0) root_sh = h.ld(0);
    __syncthreads();
    heap_stream(vec, n, c_fill, al, [&](int64_t c0, const float (&x)[4]) -> bool {
        const uint32_t cm = heap_cands(n, c0, tc, x);
        const uint32_t rk = hkey(root_sh);
        uint32_t hm = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) hm |= (uint32_t)(((cm >> j) & 1u) && abs_key(x[j]) > rk) << j;
        if (skip > 0) {   // the chunk where the fill ended: its first `skip` candidates are in the heap
            uint64_t tot;
            uint64_t r = block_exclusive_scan((uint64_t)__popc(cm), lds16, &tot);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((cm >> j) & 1u) {
                    if ((int64_t)r < skip) hm &= ~(1u << j);
                    ++r;
                }
            skip = 0;
        }
        if (!__syncthreads_or(hm != 0)) return true;
        uint64_t htot;
        const uint64_t hb = block_exclusive_scan((uint64_t)__popc(hm), lds16, &htot);
        uint64_t q = hb;
        // hot entries carry the element's offset in this chunk (< kHeapChunk)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((hm >> j) & 1u) hot[q++] = ((uint64_t)abs_key(x[j]) << kHeapKeyShift) | (uint64_t)(4 * tid + j);
        __syncthreads();
        if (tid < kWave) {   // wave 0: comp(candidate, top) is "strictly greater"
            uint64_t root = root_sh;
            for (uint64_t i = 0; i < htot; ++i) {
                const uint64_t hv = hot[i];
                if (hkey(hv) > hkey(root)) {
                    const int64_t e = c0 + (int64_t)(hv & kHeapIdxMask);
                    const uint64_t slot = root & kHeapIdxMask;   // the popped root's slot is recycled
                    if (wide && tid == 0) side[slot] = e;
                    const uint64_t v = (hv & ~kHeapIdxMask) | (uint64_t)(wide ? (int64_t)slot : e);
                    root = heap_replace_root(h, k, v);
                }
            }
            if (tid == 0) root_sh = root;
        }
        __syncthreads();
        return true;
    });
    // ---- sort_heap: k - 1 pops by wave 0
    if (tid < kWave) {
        for (int64_t last = k - 1; last >= 1; --last) {
            const uint64_t v = h.ld(last);
            const uint64_t root = h.ld(0);
            if (tid == 0) h.st(last, root);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            (void)heap_replace_root(h, last, v);
        }
    }
    __syncthreads();
    // ---- emit: payload slot p <- node p
    if (tid < kWave) {
        const long long b = out_base(w, t);
        if (tid == 0) obase_s = b;
    }
    __syncthreads();
    for (int64_t p = tid; p < k; p += kNthThreads) {
        const int64_t lo = (int64_t)(h.ld(p) & kHeapIdxMask);
        const int64_t li = wide ? side[lo] : lo;
        emit_one(o, d, obase_s + p, li, vec[li]);
    }
}

// K5 / K5b, one workgroup per tensor: the reference's resample topk replayed on the
// gathered candidates (introselect.hpp: nth_element), or — partial_sort path — heap
// select + sort_heap over vec, which also emits. They share one LDS area.
static_assert(kK5SmemBytes <= 160 * 1024 - 1024, "K5 / K5b LDS");
}  // namespace dgc
