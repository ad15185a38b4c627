// K0: local gradient clipping (dgc/clip_grad.py:10-42) — the statistic of every tensor,
// the coefficient from it, and the in-place clip of the module functions. The fused
// clip is K1's (compensate.hip, select_k1.hpp: clip1 in dgc_common.hpp).
//
// Statistics: torch's CPU norm sums in an order that depends on its thread count and
// vector width, so the reference has no fixed answer to reproduce; this one is fixed by
// the tensor's numel alone. Element e of a tensor belongs to partial e / kStatChunk, and
// inside it to lane (e % 1024) / 4 and run position (e / 1024, e % 4) whatever the
// pointer's alignment (a misaligned tensor takes the same elements with scalar loads).
// A lane adds its 16 squares in element order, the workgroup folds the lanes in a fixed
// tree, and the second kernel adds a tensor's partials — lane l takes partials l, l +
// 256, ... in order, then the same tree. Squares and sums are fp64: a float's square is
// exact there, and the sum of n <= 2^20 of them is within n * 2^-53 of the true one.
// The maximum has no order to fix; NaN wins, as in torch's max.
#include <algorithm>
#include <cmath>

#include "dispatch.hpp"
#include "payload.hpp"

namespace dgc {

constexpr int kStatPerLane = 16;
constexpr int kStatChunk = kBlock * kStatPerLane;   // elements per partial
constexpr int kClipMax = 64;                        // tensors per launch (table in the arguments)
constexpr int kClipPerThread = 4;

template <typename T>
struct ClipChunkT {
    int32_t count, first;                // tensors [first, first + count) of the call
    int32_t bstart[kClipMax + 1];        // first workgroup of each tensor (prefix)
    T* src[kClipMax];
    int64_t n[kClipMax];
    int64_t poff[kClipMax];              // stats: the tensor's first partial
};
using ClipChunk = ClipChunkT<float>;
using ClipChunk16 = ClipChunkT<const uint16_t>;   // K0-16: bf16 / fp16 sources

__device__ __forceinline__ float nan_max(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }

// The workgroup's fold: lanes of a wave by halving distance, then the four waves in
// order. Every thread returns the same value.
template <bool MAX>
__device__ __forceinline__ double block_fold(double x) {
    __shared__ double part[kBlock / 64];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double y = __shfl_down(x, d, 64);
        x = MAX ? (double)nan_max((float)x, (float)y) : x + y;
    }
    __syncthreads();   // a second fold in the same kernel: the slots are free again
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = x;
    __syncthreads();
    double r = part[0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) r = MAX ? (double)nan_max((float)r, (float)part[w]) : r + part[w];
    return r;
}

template <bool MAX, bool ROUND16>
__global__ void __launch_bounds__(kBlock) k_stat_partial(ClipChunk c, double* __restrict__ part) {
    const int b = (int)blockIdx.x;
    const int t = chunk_of(c, b);
    const float* __restrict__ src = c.src[t];
    const int64_t n = c.n[t];
    const int64_t j = b - c.bstart[t];
    const bool vec = aligned16(src);
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < kStatPerLane / 4; ++u) {
        const int64_t e = j * kStatChunk + (int64_t)u * (kBlock * 4) + 4 * (int64_t)threadIdx.x;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec && e + 3 < n) {
            const float4 v = ld_nt(reinterpret_cast<const float4*>(src + e));
            x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (e + q < n) x[q] = src[e + q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            // past the end: +0.0, which changes neither a sum of squares nor a max of |x|
            const float y = ROUND16 ? f16_to_f32(f32_to_f16(x[q])) : x[q];
            if (MAX) acc = (double)nan_max((float)acc, fabsf(y));
            else acc += (double)y * (double)y;
        }
    }
    acc = block_fold<MAX>(acc);
    if (threadIdx.x == 0) part[c.poff[t] + j] = acc;
}

// K0-16: the same partials from a bf16 / fp16 source. Element e keeps its partial, lane and
// position, so the fp64 sum is the one k_stat_partial forms on the widened tensor. A lane's
// four groups are 8-B non-temporal loads (the width K1-16 streams), all issued before the
// first is used; a source that is not 8-B aligned, and the group the tensor ends in, take
// the same elements by 2-B loads, none past numel. (One 8-KB partial per workgroup: at 1e9
// elements the pass takes 0.57 ms, about K0's time per ELEMENT (0.65 ms), so it is not the
// bytes that bound it; two partials per workgroup with all eight loads in flight measured
// 0.64 ms and was not kept. DESIGN.md §4 "Gradient clipping".)
typedef uint32_t u2v __attribute__((ext_vector_type(2)));

template <int DT, bool MAX>
__global__ void __launch_bounds__(kBlock) k_stat_partial16(ClipChunk16 c, double* __restrict__ part) {
    const int b = (int)blockIdx.x;
    const int t = chunk_of(c, b);
    DGC_GLB const uint16_t* src = glb(c.src[t]);
    const int64_t n = c.n[t];
    const int64_t j = b - c.bstart[t];
    const bool vec = (reinterpret_cast<uintptr_t>(c.src[t]) & 7u) == 0;
    uint32_t lo[kStatPerLane / 4], hi[kStatPerLane / 4];
#pragma unroll
    for (int u = 0; u < kStatPerLane / 4; ++u) {
        const int64_t e = j * kStatChunk + (int64_t)u * (kBlock * 4) + 4 * (int64_t)threadIdx.x;
        lo[u] = hi[u] = 0u;   // past the end: +0
        if (vec && e + 3 < n) {
            const u2v v = __builtin_nontemporal_load(reinterpret_cast<DGC_GLB const u2v*>(src + e));
            lo[u] = v[0], hi[u] = v[1];
        } else {
            if (e < n) lo[u] = (uint32_t)src[e];
            if (e + 1 < n) lo[u] |= (uint32_t)src[e + 1] << 16;
            if (e + 2 < n) hi[u] = (uint32_t)src[e + 2];
            if (e + 3 < n) hi[u] |= (uint32_t)src[e + 3] << 16;
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < kStatPerLane / 4; ++u) {
        const uint16_t h[4] = {(uint16_t)(lo[u] & 0xFFFFu), (uint16_t)(lo[u] >> 16), (uint16_t)(hi[u] & 0xFFFFu),
                               (uint16_t)(hi[u] >> 16)};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float y = h16_to_f32<DT>(h[q]);
            if (MAX) acc = (double)nan_max((float)acc, fabsf(y));
            else acc += (double)y * (double)y;
        }
    }
    acc = block_fold<MAX>(acc);
    if (threadIdx.x == 0) part[c.poff[t] + j] = acc;
}

// RDT: the result rounded to fp32, then (a 16-bit source, K0-16) to that dtype, and stored
// as the fp32 image of the dtype's value: what an ATen reduction leaves in a 0-dim tensor.
template <bool MAX, int RDT = DGC_F32, typename C = ClipChunk>
__global__ void __launch_bounds__(kBlock)
k_stat_final(C c, const double* __restrict__ part, float* __restrict__ stats, int root) {
    const int t = (int)blockIdx.x;
    const int64_t np = ceil_div(c.n[t], (int64_t)kStatChunk);
    const double* __restrict__ p = part + c.poff[t];
    double acc = 0.0;
    // lane l folds partials l, l + 256, ... in that order; eight loads in flight at a time
    // (a slot past the end reads as +0.0, which changes neither fold)
    for (int64_t i = threadIdx.x; i < np; i += (int64_t)kBlock * 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t q = i + (int64_t)u * kBlock;
            v[u] = q < np ? p[q] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (MAX) acc = (double)nan_max((float)acc, (float)v[u]);
            else acc += v[u];
        }
    }
    acc = block_fold<MAX>(acc);
    if (threadIdx.x == 0) {
        const float r = (float)(root ? sqrt(acc) : acc);
        stats[c.first + t] = RDT == DGC_F32 ? r : round16<RDT == DGC_F32 ? DGC_BF16 : RDT>(r);
    }
}

template <typename T>
static int clip_chunk(T* const* srcs, const int64_t* numels, int32_t t0, int32_t total, int64_t per_block,
                      ClipChunkT<T>& c, int64_t& blocks, const char* who) {
    constexpr unsigned align = sizeof(T);
    c = ClipChunkT<T>{};
    c.first = t0;
    c.count = std::min<int32_t>(kClipMax, total - t0);
    blocks = 0;
    for (int i = 0; i < c.count; ++i) {
        const int64_t n = numels[t0 + i];
        if (n < 0 || (n > 0 && !srcs[t0 + i])) DGC_FAIL(DGC_ERR_INVALID, "%s: tensor %d: bad pointer or size", who, t0 + i);
        if (reinterpret_cast<uintptr_t>(srcs[t0 + i]) & (align - 1))
            DGC_FAIL(DGC_ERR_INVALID, "%s: tensor %d is not %u-B aligned", who, t0 + i, align);
        c.bstart[i] = (int32_t)blocks;
        c.src[i] = srcs[t0 + i];
        c.n[i] = n;
        blocks += ceil_div(n, per_block);
        if (blocks > 0x7FFFFFFFLL) DGC_FAIL(DGC_ERR_INVALID, "%s: too many elements", who);
    }
    c.bstart[c.count] = (int32_t)blocks;
    return DGC_OK;
}

static int64_t stat_partials(const int64_t* numels, int32_t count) {
    int64_t p = 0;
    for (int32_t t = 0; t < count; ++t) {
        if (numels[t] < 0) return -1;
        p += ceil_div(numels[t], (int64_t)kStatChunk);
    }
    return p;
}

size_t grad_stats_ws(const int64_t* numels, int32_t count) {
    if (count < 0 || (count > 0 && !numels)) return 0;
    const int64_t p = stat_partials(numels, count);
    if (p < 0) return 0;
    return align_up((size_t)std::max<int64_t>(p, 1) * sizeof(double), 256);
}

int grad_stats(const float* const* srcs, const int64_t* numels, int32_t count, int32_t kind, int32_t round_to,
               float* stats, void* ws, size_t ws_bytes, hipStream_t st) {
    if (count < 0 || (count > 0 && (!srcs || !numels || !stats))) DGC_FAIL(DGC_ERR_INVALID, "dgc_grad_stats: null argument");
    if (kind != DGC_STAT_SUMSQ && kind != DGC_STAT_NORM2 && kind != DGC_STAT_ABSMAX)
        DGC_FAIL(DGC_ERR_INVALID, "dgc_grad_stats: kind %d", (int)kind);
    if (round_to != DGC_F32 && round_to != DGC_F16) DGC_FAIL(DGC_ERR_DTYPE, "dgc_grad_stats: round_to");
    if (count == 0) return DGC_OK;
    if (stat_partials(numels, count) < 0) DGC_FAIL(DGC_ERR_INVALID, "dgc_grad_stats: negative numel");
    const size_t need = grad_stats_ws(numels, count);
    if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 255))
        DGC_FAIL(DGC_ERR_WORKSPACE, "dgc_grad_stats: workspace needs %zu bytes, 256-B aligned", need);
    double* part = static_cast<double*>(ws);
    const bool mx = kind == DGC_STAT_ABSMAX, r16 = round_to == DGC_F16;
    int64_t poff = 0;
    for (int32_t t0 = 0; t0 < count; t0 += kClipMax) {
        ClipChunk c;
        int64_t blocks;
        DGC_TRY(clip_chunk(const_cast<float* const*>(srcs), numels, t0, count, kStatChunk, c, blocks, "dgc_grad_stats"));
        for (int i = 0; i < c.count; ++i) {
            c.poff[i] = poff;
            poff += ceil_div(c.n[i], (int64_t)kStatChunk);
        }
        const dim3 bd(kBlock);
        if (blocks > 0) {
            const dim3 gd((unsigned)blocks);
            with_bool(mx, [&](auto MAX) { with_bool(r16, [&](auto R16) {
                hipLaunchKernelGGL((k_stat_partial<MAX(), R16()>), gd, bd, 0, st, c, part); }); });
            DGC_LAUNCHED();
        }
        const dim3 gf((unsigned)c.count);
        with_bool(mx, [&](auto MAX) {
            hipLaunchKernelGGL((k_stat_final<MAX()>), gf, bd, 0, st, c, part, stats, kind == DGC_STAT_NORM2 ? 1 : 0); });
        DGC_LAUNCHED();
    }
    return DGC_OK;
}

// `clip_coef = max_norm / (total_norm + 1e-6)` on a 0-dim fp32 tensor: the add takes the
// scalar as fl32(1e-6), and a Python float divided by a tensor is torch's
// reciprocal().mul(max_norm) — 1 / x rounded, then the product rounded.
__global__ void __launch_bounds__(kBlock)
k_clip_coefs(const float* stats, int32_t count, int mode, float max_norm, float* clip) {
    const int t = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (t >= count) return;
    float s = stats[t];
    // torch.sqrt's correctly rounded fp32 root: the fp64 root rounded to fp32 is that
    // (53 >= 2 * 24 + 2 bits: the double rounding is innocuous)
    if (mode != DGC_COEF_NORM) s = (float)sqrt((double)s);
    clip[t] = mode == DGC_COEF_GLOBAL_VALUE ? s : __fmul_rn(__fdiv_rn(1.f, __fadd_rn(s, 1e-6f)), max_norm);
}

int clip_coefs(const float* stats, int32_t count, int32_t mode, float max_norm, float* clip, hipStream_t st) {
    if (count < 0 || (count > 0 && (!stats || !clip))) DGC_FAIL(DGC_ERR_INVALID, "dgc_clip_coefs: null argument");
    if (mode != DGC_COEF_NORM && mode != DGC_COEF_GLOBAL_VALUE && mode != DGC_COEF_GLOBAL_NORM2)
        DGC_FAIL(DGC_ERR_INVALID, "dgc_clip_coefs: mode %d", (int)mode);
    if (count == 0) return DGC_OK;
    hipLaunchKernelGGL(k_clip_coefs, dim3((unsigned)ceil_div(count, kBlock)), dim3(kBlock), 0, st, stats, count,
                       (int)mode, max_norm, clip);
    DGC_LAUNCHED();
    return DGC_OK;
}

// K0-16: the statistic of bf16 / fp16 tensors, as torch leaves it in a 0-dim tensor of the
// dtype (x.norm(2), x.abs().max()): the fp64 result rounded to fp32, then to the dtype.
int grad_stats16(const void* const* srcs, const int64_t* numels, int32_t count, int32_t kind, int32_t dtype,
                 float* stats, void* ws, size_t ws_bytes, hipStream_t st) {
    if (count < 0 || (count > 0 && (!srcs || !numels || !stats)))
        DGC_FAIL(DGC_ERR_INVALID, "dgc_grad_stats16: null argument");
    if (kind == DGC_STAT_SUMSQ)
        DGC_FAIL(DGC_ERR_INVALID, "dgc_grad_stats16: DGC_STAT_SUMSQ (the global variants) is not taken on 16-bit tensors");
    if (kind != DGC_STAT_NORM2 && kind != DGC_STAT_ABSMAX) DGC_FAIL(DGC_ERR_INVALID, "dgc_grad_stats16: kind %d", (int)kind);
    if (!is16(dtype))
        DGC_FAIL(DGC_ERR_DTYPE, "dgc_grad_stats16: dtype must be DGC_BF16 or DGC_F16 (got %d)", (int)dtype);
    if (count == 0) return DGC_OK;
    if (stat_partials(numels, count) < 0) DGC_FAIL(DGC_ERR_INVALID, "dgc_grad_stats16: negative numel");
    const size_t need = grad_stats_ws(numels, count);
    if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 255))
        DGC_FAIL(DGC_ERR_WORKSPACE, "dgc_grad_stats16: workspace needs %zu bytes, 256-B aligned", need);
    // the table's pointers before the first launch (clip_chunk looks at a chunk as it is launched)
    for (int32_t t = 0; t < count; ++t) {
        if (numels[t] > 0 && !srcs[t]) DGC_FAIL(DGC_ERR_INVALID, "dgc_grad_stats16: tensor %d: bad pointer or size", t);
        if (reinterpret_cast<uintptr_t>(srcs[t]) & 1u)
            DGC_FAIL(DGC_ERR_INVALID, "dgc_grad_stats16: tensor %d is not 2-B aligned", t);
    }
    if (stat_partials(numels, count) > 0x7FFFFFFFLL) DGC_FAIL(DGC_ERR_INVALID, "dgc_grad_stats16: too many elements");
    const uint16_t* const* src16 = reinterpret_cast<const uint16_t* const*>(srcs);   // the ABI's void pointers
    double* part = static_cast<double*>(ws);
    int64_t poff = 0;
    for (int32_t t0 = 0; t0 < count; t0 += kClipMax) {
        ClipChunk16 c;
        int64_t blocks;
        DGC_TRY(clip_chunk(src16, numels, t0, count, kStatChunk, c, blocks, "dgc_grad_stats16"));
        for (int i = 0; i < c.count; ++i) {
            c.poff[i] = poff;
            poff += ceil_div(c.n[i], (int64_t)kStatChunk);
        }
        const dim3 bd(kBlock), gd((unsigned)blocks), gf((unsigned)c.count);
        with_h16(dtype, [&](auto DT) { with_bool(kind == DGC_STAT_ABSMAX, [&](auto MAX) {
            if (blocks > 0) hipLaunchKernelGGL((k_stat_partial16<DT(), MAX()>), gd, bd, 0, st, c, part);
            // the final's last argument: the root of the sum of squares (the 2-norm)
            hipLaunchKernelGGL((k_stat_final<MAX(), DT(), ClipChunk16>), gf, bd, 0, st, c, part, stats, MAX() ? 0 : 1); }); });
        DGC_LAUNCHED();
    }
    return DGC_OK;
}

// `max_norm / (total_norm + 1e-6)` on a 0-dim tensor of a 16-bit dtype: the add, the
// reciprocal and the product each computed in fp32 and rounded to the dtype.
template <int DT>
__global__ void __launch_bounds__(kBlock)
k_clip_coefs16(const float* stats, int32_t count, float max_norm, float* clip) {
    const int t = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (t >= count) return;
    const float total = round16<DT>(__fadd_rn(stats[t], 1e-6f));
    const float inv = round16<DT>(__fdiv_rn(1.f, total));
    clip[t] = round16<DT>(__fmul_rn(inv, max_norm));
}

int clip_coefs16(const float* stats, int32_t count, float max_norm, int32_t dtype, float* clip, hipStream_t st) {
    if (count < 0 || (count > 0 && (!stats || !clip))) DGC_FAIL(DGC_ERR_INVALID, "dgc_clip_coefs16: null argument");
    if (!is16(dtype))
        DGC_FAIL(DGC_ERR_DTYPE, "dgc_clip_coefs16: dtype must be DGC_BF16 or DGC_F16 (got %d)", (int)dtype);
    if (count == 0) return DGC_OK;
    const dim3 gd((unsigned)ceil_div(count, kBlock)), bd(kBlock);
    with_h16(dtype, [&](auto DT) { hipLaunchKernelGGL(k_clip_coefs16<DT()>, gd, bd, 0, st, stats, count, max_norm, clip); });
    DGC_LAUNCHED();
    return DGC_OK;
}

template <int CLIP>
__global__ void __launch_bounds__(kBlock) k_clip_apply(ClipChunk c, ClipArg ca) {
    const int b = (int)blockIdx.x;
    const int t = chunk_of(c, b);
    float* __restrict__ x = c.src[t];
    const int64_t n = c.n[t];
    const float cf = clip_coef<CLIP>(ca, c.first + t);
    const int64_t e0 = ((int64_t)(b - c.bstart[t]) * kBlock) * kClipPerThread + threadIdx.x;
#pragma unroll
    for (int j = 0; j < kClipPerThread; ++j) {
        const int64_t e = e0 + (int64_t)j * kBlock;
        if (e >= n) break;
        x[e] = clip1<CLIP>(x[e], cf);
    }
}

int clip_apply(float* const* tensors, const int64_t* numels, int32_t count, int32_t kind, const float* clip,
               float value, hipStream_t st) {
    if (count < 0 || (count > 0 && (!tensors || !numels))) DGC_FAIL(DGC_ERR_INVALID, "dgc_clip_apply: null argument");
    if (kind != DGC_CLIP_SCALE && kind != DGC_CLIP_CLAMP) DGC_FAIL(DGC_ERR_INVALID, "dgc_clip_apply: clip kind %d", (int)kind);
    if (kind == DGC_CLIP_SCALE && !clip) DGC_FAIL(DGC_ERR_INVALID, "dgc_clip_apply: DGC_CLIP_SCALE needs the coefficient table");
    for (int32_t t0 = 0; t0 < count; t0 += kClipMax) {
        ClipChunk c;
        int64_t blocks;
        DGC_TRY(clip_chunk(tensors, numels, t0, count, (int64_t)kBlock * kClipPerThread, c, blocks, "dgc_clip_apply"));
        if (blocks == 0) continue;
        const dim3 gd((unsigned)blocks), bd(kBlock);
        const ClipArg ca{clip, value};
        with_clip_on(kind, [&](auto CLIP) { hipLaunchKernelGGL((k_clip_apply<CLIP()>), gd, bd, 0, st, c, ca); });
        DGC_LAUNCHED();
    }
    return DGC_OK;
}

}  // namespace dgc

extern "C" size_t dgc_grad_stats_workspace(const int64_t* numels, int32_t count) {
    return dgc::grad_stats_ws(numels, count);
}

extern "C" int dgc_grad_stats(const float* const* srcs, const int64_t* numels, int32_t count, int32_t kind,
                              int32_t round_to, float* stats, void* ws, size_t ws_bytes, void* stream) {
    return dgc::grad_stats(srcs, numels, count, kind, round_to, stats, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int dgc_clip_coefs(const float* stats, int32_t count, int32_t mode, float max_norm, float* clip,
                              void* stream) {
    return dgc::clip_coefs(stats, count, mode, max_norm, clip, static_cast<hipStream_t>(stream));
}

extern "C" int dgc_clip_apply(float* const* tensors, const int64_t* numels, int32_t count, int32_t clip_kind,
                              const float* clip, float clip_value, void* stream) {
    return dgc::clip_apply(tensors, numels, count, clip_kind, clip, clip_value, static_cast<hipStream_t>(stream));
}

extern "C" int dgc_grad_stats16(const void* const* srcs, const int64_t* numels, int32_t count, int32_t kind,
                                int32_t dtype, float* stats, void* ws, size_t ws_bytes, void* stream) {
    return dgc::grad_stats16(srcs, numels, count, kind, dtype, stats, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int dgc_clip_coefs16(const float* stats, int32_t count, float max_norm, int32_t dtype, float* clip,
                                void* stream) {
    return dgc::clip_coefs16(stats, count, max_norm, dtype, clip, static_cast<hipStream_t>(stream));
}
