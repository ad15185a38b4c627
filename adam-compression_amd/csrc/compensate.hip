// K1: momentum correction + velocity accumulation, with the strided sample of
// |velocity| fused into the same streaming pass; K2: standalone sampling.
//
// Reference: DGCSGDMemory.compensate (dgc/memory.py:50-70) and the sampling of
// DGCCompressor._sparsify (dgc/compression.py:113-121).
//
// Bit-exactness: the reference issues separate ATen ops (add_, mul_), so every
// intermediate rounds to fp32. This file is built with -ffp-contract=off and uses
// __fadd_rn / __fmul_rn so no multiply-add is ever fused:
//   nesterov: mmt = (mmt + g) * m ;  vec = (vec + mmt) + g   [accumulate]
//                                     out = mmt + g           [dense branch]
//   plain:    mmt = mmt * m + g   ;  vec = vec + mmt         [accumulate]
//                                     out = mmt               [dense branch]
//
// HBM: 20 B/element (read g, mmt, vec; write mmt, vec), non-temporal 16-B accesses,
// one float4 per lane in one-shot block chunks. The sample |vec[start + q*stride]|
// is written from registers, saving a strided re-read of vec (which would touch
// ~1/3 of its lines).
#include <algorithm>

#include "dispatch.hpp"
#include "payload.hpp"

namespace dgc {


// Vector path: all pointers 16-B aligned. One-shot chunks (no grid stride): block b
// owns float4 [256b, 256b + 256), lanes contiguous, non-temporal 16-B loads and
// stores. Measured on MI355X this shape streams 3R2W at 5.86 TB/s against 4.8 TB/s
// for the grid-stride loop (tools/membench.hip). The sample bookkeeping is per
// block: (q0, r0) = floor/mod(4*256b - start, stride) once, then a 32-bit divide
// of the lane's small offset.
template <bool NEST, bool ACC, bool SAMPLE, int CLIP>
__global__ void __launch_bounds__(kBlock)
k_compensate4(const float4* __restrict__ g, float4* __restrict__ mmt, float4* __restrict__ vec,
              float4* __restrict__ out, int64_t n4, float mom, SampleSpec sp, int wt, ClipArg ca) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= n4) return;
    const float4 gv = clip4<CLIP>(ld_nt(g + v), clip_coef<CLIP>(ca, 0));
    float4 mv = ld_nt(mmt + v);
    float4 vv = ACC ? ld_nt(vec + v) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 ov;
    ov.x = comp1<NEST, ACC>(gv.x, mv.x, vv.x, mom);
    ov.y = comp1<NEST, ACC>(gv.y, mv.y, vv.y, mom);
    ov.z = comp1<NEST, ACC>(gv.z, mv.z, vv.z, mom);
    ov.w = comp1<NEST, ACC>(gv.w, mv.w, vv.w, mom);
    st_stream(mmt + v, mv, wt);
    if (ACC)
        st_stream(vec + v, vv, wt);
    else
        st_stream(out + v, ov, wt);
    if (SAMPLE) {
        int64_t q0, r0;
        floor_divmod_fast(4 * ((int64_t)blockIdx.x * kBlock) - sp.start, sp.stride, sp.inv_stride, q0, r0);
        // element 4v+j is a sample iff (r + j) % stride == 0, with r = (r0 + 4*tid) mod stride
        const uint32_t t = (uint32_t)r0 + 4u * threadIdx.x;
        const uint32_t s32 = (uint32_t)sp.stride;
        uint32_t q1, r;
        divmod_u32(t, s32, sp.inv_stride_f, q1, r);
        const uint32_t j = r == 0 ? 0u : s32 - r;
        if (j < 4) {
            const int64_t qi = q0 + q1 + (r == 0 ? 0 : 1);
            if (qi >= 0 && qi < sp.count) {
                const float x = j == 0 ? ov.x : j == 1 ? ov.y : j == 2 ? ov.z : ov.w;
                sp.out[qi] = fabsf(x);
            }
        }
    }
}

// Scalar path: any alignment, any stride; also used for the < 4-element tail.
template <bool NEST, bool ACC, bool SAMPLE, int CLIP>
__global__ void __launch_bounds__(kBlock)
k_compensate1(const float* __restrict__ g, float* __restrict__ mmt, float* __restrict__ vec,
              float* __restrict__ out, int64_t begin, int64_t n, float mom, SampleSpec sp, ClipArg ca) {
    const float cf = clip_coef<CLIP>(ca, 0);
    for (int64_t i = begin + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * kBlock) {
        float mv = mmt[i];
        float vv = ACC ? vec[i] : 0.f;
        const float ov = comp1<NEST, ACC>(clip1<CLIP>(g[i], cf), mv, vv, mom);
        mmt[i] = mv;
        if (ACC)
            vec[i] = vv;
        else
            out[i] = ov;
        if (SAMPLE && i >= sp.start) {
            const int64_t d = i - sp.start;
            if (d % sp.stride == 0 && d / sp.stride < sp.count) sp.out[d / sp.stride] = fabsf(ov);
        }
    }
}

__global__ void __launch_bounds__(kBlock)
k_sample_strided(const float* __restrict__ vec, int64_t start, int64_t stride, int64_t count,
                 float* __restrict__ out) {
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < count;
         q += (int64_t)gridDim.x * kBlock)
        out[q] = fabsf(vec[start + q * stride]);
}

__global__ void __launch_bounds__(kBlock)
k_sample_gather(const float* __restrict__ vec, const int64_t* __restrict__ idx, int64_t count,
                float* __restrict__ out) {
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < count;
         q += (int64_t)gridDim.x * kBlock)
        out[q] = fabsf(vec[idx[q]]);
}

// DGCSGDMemory.update (dgc/memory.py:72-77) on its own: zero the transmitted slots.
template <typename I>
__global__ void __launch_bounds__(kBlock)
k_mask(float* __restrict__ mmt, float* __restrict__ vec, const I* __restrict__ idx, int64_t count,
       int64_t n, int* bad) {
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < count;
         q += (int64_t)gridDim.x * kBlock) {
        int64_t i = (int64_t)idx[q];
        if (i < 0) i += n;             // torch index_fill_ wraps negative indices
        if (i < 0 || i >= n) {
            raise_flag(bad);
            continue;
        }
        if (mmt) mmt[i] = 0.f;
        vec[i] = 0.f;
    }
}

int sample_strided_launch(const float* vec, int64_t start, int64_t stride, int64_t count, float* out,
                          hipStream_t s) {
    if (count <= 0) return DGC_OK;
    hipLaunchKernelGGL(k_sample_strided, dim3(grid_for(count)), dim3(kBlock), 0, s, vec, start, stride, count, out);
    DGC_LAUNCHED();
    return DGC_OK;
}

template <bool NEST, bool ACC, int CLIP>
static int launch_comp(const float* g, float* m, float* v, float* o, int64_t n, float mom,
                       SampleSpec sp, ClipArg ca, hipStream_t st) {
    const bool sample = sp.out != nullptr;
    const bool vec_ok = aligned16(g) && aligned16(m) && (ACC ? aligned16(v) : aligned16(o)) &&
                        (!sample || (sp.stride >= 4 && sp.stride < (1LL << 30)));
    int64_t done = 0;
    if (vec_ok) {
        const int64_t n4 = n / 4;
        if (n4 > 0) {
            const int64_t grid = ceil_div(n4, kBlock);
            if (grid > 0x7FFFFFFFLL) DGC_FAIL(DGC_ERR_INVALID, "dgc_compensate: n too large");
            auto g4 = reinterpret_cast<const float4*>(g);
            auto m4 = reinterpret_cast<float4*>(m);
            auto v4 = reinterpret_cast<float4*>(v);
            auto o4 = reinterpret_cast<float4*>(o);
            with_bool(sample, [&](auto SAMPLE) {
                hipLaunchKernelGGL((k_compensate4<NEST, ACC, SAMPLE(), CLIP>), dim3((unsigned)grid), dim3(kBlock), 0, st,
                                   g4, m4, v4, o4, n4, mom, sp, (int)write_through(n), ca); });
            DGC_LAUNCHED();
        }
        done = n4 * 4;
    }
    if (done < n) {
        const int grid = grid_for(n - done);
        with_bool(sample, [&](auto SAMPLE) {
            hipLaunchKernelGGL((k_compensate1<NEST, ACC, SAMPLE(), CLIP>), dim3(grid), dim3(kBlock), 0, st,
                               g, m, v, o, done, n, mom, sp, ca); });
        DGC_LAUNCHED();
    }
    return DGC_OK;
}

// ---- the dense tensors of a step (dgc/compression.py:173-177, 195-198) ----
// Multi-tensor gather with the wire cast: dst[off_t + i] = cast(src_t[i]) for up to
// kMtMax tensors per launch (their table rides in the kernel arguments): the dense
// gradients of a step, wherever autograd put them, into one allreduce buffer — fp16
// when the compressor casts (`tensor.type(torch.float16)`), else fp32. One launch where
// a copy per parameter was one ATen launch each (107 for ResNet-50).
constexpr int kMtMax = 64;
constexpr int kMtPerThread = 4;
struct MtChunk {
    int32_t count, dtype;                // dtype: DGC_F32 / DGC_F16 / DGC_BF16 of dst
    int32_t bstart[kMtMax + 1];          // first workgroup of each tensor (prefix)
    const float* src[kMtMax];
    int64_t n[kMtMax];
    int64_t off[kMtMax];
};

__global__ void __launch_bounds__(kBlock) k_gather_cast(MtChunk c, void* __restrict__ dst) {
    int lo = 0, hi = c.count - 1;   // the tensor of this workgroup: bstart[t] <= b < bstart[t + 1]
    const int b = (int)blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (c.bstart[mid] <= b) lo = mid; else hi = mid - 1;
    }
    const int t = lo;
    const float* __restrict__ src = c.src[t];
    const int64_t n = c.n[t], off = c.off[t];
    const int64_t e0 = ((int64_t)(b - c.bstart[t]) * kBlock) * kMtPerThread + threadIdx.x;
#pragma unroll
    for (int j = 0; j < kMtPerThread; ++j) {
        const int64_t e = e0 + (int64_t)j * kBlock;
        if (e >= n) break;
        const float x = src[e];
        if (c.dtype == DGC_F16)
            static_cast<uint16_t*>(dst)[off + e] = f32_to_f16(x);
        else if (c.dtype == DGC_BF16)
            static_cast<uint16_t*>(dst)[off + e] = f32_to_bf16(x);
        else
            static_cast<float*>(dst)[off + e] = x;
    }
}

// compensate(accumulate=False) of the exchanged dense gradient (dgc/memory.py:50-70 on
// what decompress hands it, dgc/compression.py:195-198): the source is the allreduce
// buffer — fp32, or fp16 widened exactly as `tensor.type(vdtype)` does — or, ROUND16, an
// fp32 gradient rounded to fp16 and back (a one-rank exchange of an fp16 wire, with no
// buffer in between). div != 1: the source is the allreduce's SUM and the Average's
// `div_(W)` happens here, in the wire dtype as torch does it (fp32 quotient, rounded to
// fp16 for an fp16 wire) — no ATen launch. Four elements per thread; the dense tensors
// are small.
template <bool NEST, int SRC>   // SRC: 0 fp32, 1 fp16, 2 fp32 rounded through fp16
__global__ void __launch_bounds__(kBlock)
k_compensate_wire(const void* __restrict__ src, float* __restrict__ mmt, float* __restrict__ out, int64_t n,
                  float mom, float div) {
    const int64_t e0 = (int64_t)blockIdx.x * kBlock * 4 + threadIdx.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t e = e0 + (int64_t)j * kBlock;
        if (e >= n) break;
        float g;
        if (SRC == 1) {
            g = f16_to_f32(static_cast<const uint16_t*>(src)[e]);
            if (div != 1.f) g = f16_to_f32(f32_to_f16(__fdiv_rn(g, div)));
        } else if (SRC == 2) {
            g = f16_to_f32(f32_to_f16(static_cast<const float*>(src)[e]));
        } else {
            g = static_cast<const float*>(src)[e];
            if (div != 1.f) g = __fdiv_rn(g, div);
        }
        float m = mmt[e], v = 0.f;
        const float o = comp1<NEST, false>(g, m, v, mom);
        mmt[e] = m;
        out[e] = o;
    }
}

// compensate(accumulate=False) of up to kMtMax tensors per launch straight from their
// gradients (a one-rank exchange: nothing to gather for an allreduce), mmt and out at
// the tensors' offsets of two flat buffers; ROUND16: each gradient rounded to fp16 and
// back first (the fp16 wire's cast and decompress's widening).
template <bool NEST, bool ROUND16, int CLIP>
__global__ void __launch_bounds__(kBlock) k_compensate_mt(MtChunk c, float* __restrict__ mmt, float* __restrict__ out,
                                                          float mom, ClipArg ca, int t0) {
    int lo = 0, hi = c.count - 1;
    const int b = (int)blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (c.bstart[mid] <= b) lo = mid; else hi = mid - 1;
    }
    const int t = lo;
    const float* __restrict__ src = c.src[t];
    const int64_t n = c.n[t], off = c.off[t];
    const float cf = clip_coef<CLIP>(ca, t0 + t);
    const int64_t e0 = ((int64_t)(b - c.bstart[t]) * kBlock) * kMtPerThread + threadIdx.x;
#pragma unroll
    for (int j = 0; j < kMtPerThread; ++j) {
        const int64_t e = e0 + (int64_t)j * kBlock;
        if (e >= n) break;
        const float g = clip1<CLIP>(ROUND16 ? f16_to_f32(f32_to_f16(src[e])) : src[e], cf);
        float m = mmt[off + e], v = 0.f;
        const float o = comp1<NEST, false>(g, m, v, mom);
        mmt[off + e] = m;
        out[off + e] = o;
    }
}

// The tensor table of one launch: tensors [t0, t0 + count) of the host arrays.
static int mt_chunk(const float* const* srcs, const int64_t* numels, const int64_t* offsets, int32_t t0,
                    int32_t total, MtChunk& c, int64_t& blocks, const char* who) {
    c = MtChunk{};
    c.count = std::min<int32_t>(kMtMax, total - t0);
    blocks = 0;
    for (int i = 0; i < c.count; ++i) {
        const int64_t n = numels[t0 + i];
        if (n < 0 || offsets[t0 + i] < 0 || (n > 0 && !srcs[t0 + i]))
            DGC_FAIL(DGC_ERR_INVALID, "%s: tensor %d: bad pointer, size or offset", who, t0 + i);
        c.bstart[i] = (int32_t)blocks;
        c.src[i] = srcs[t0 + i];
        c.n[i] = n;
        c.off[i] = offsets[t0 + i];
        blocks += ceil_div(n, (int64_t)kBlock * kMtPerThread);
        if (blocks > 0x7FFFFFFFLL) DGC_FAIL(DGC_ERR_INVALID, "%s: too many elements", who);
    }
    c.bstart[c.count] = (int32_t)blocks;
    return DGC_OK;
}

int compensate_multi(const float* const* srcs, const int64_t* numels, const int64_t* offsets, int32_t count,
                     int32_t round_to, float* mmt, float* out, float mom, bool nesterov, int32_t clip_kind,
                     ClipArg ca, hipStream_t st) {
    if (count < 0 || (count > 0 && (!srcs || !numels || !offsets || !mmt || !out)))
        DGC_FAIL(DGC_ERR_INVALID, "dgc_compensate_multi: null argument");
    if (round_to != DGC_F32 && round_to != DGC_F16) DGC_FAIL(DGC_ERR_DTYPE, "dgc_compensate_multi: round_to");
    DGC_TRY(check_clip("dgc_compensate_multi", clip_kind, ca.tab));
    for (int32_t t0 = 0; t0 < count; t0 += kMtMax) {
        MtChunk c;
        int64_t blocks;
        DGC_TRY(mt_chunk(srcs, numels, offsets, t0, count, c, blocks, "dgc_compensate_multi"));
        if (blocks == 0) continue;
        const dim3 gd((unsigned)blocks), bd(kBlock);
        with_bool(nesterov, [&](auto NEST) { with_bool(round_to == DGC_F16, [&](auto ROUND16) {
            with_clip(clip_kind, [&](auto CLIP) {
                hipLaunchKernelGGL((k_compensate_mt<NEST(), ROUND16(), CLIP()>), gd, bd, 0, st, c, mmt, out, mom, ca, t0);
            }); }); });
        DGC_LAUNCHED();
    }
    return DGC_OK;
}

int gather_cast(const float* const* srcs, const int64_t* numels, const int64_t* offsets, int32_t count, void* dst,
                int32_t dtype, hipStream_t st) {
    if (count < 0 || (count > 0 && (!srcs || !numels || !offsets || !dst)))
        DGC_FAIL(DGC_ERR_INVALID, "dgc_gather_cast: null argument");
    if (!float_dtype_ok(dtype)) DGC_FAIL(DGC_ERR_DTYPE, "dgc_gather_cast: dtype");
    for (int32_t t0 = 0; t0 < count; t0 += kMtMax) {
        MtChunk c;
        int64_t blocks;
        DGC_TRY(mt_chunk(srcs, numels, offsets, t0, count, c, blocks, "dgc_gather_cast"));
        c.dtype = dtype;
        if (blocks == 0) continue;
        hipLaunchKernelGGL(k_gather_cast, dim3((unsigned)blocks), dim3(kBlock), 0, st, c, dst);
        DGC_LAUNCHED();
    }
    return DGC_OK;
}

int compensate_wire(const void* src, int32_t src_dtype, int32_t round_to, float* mmt, float* out, int64_t n,
                    float mom, bool nesterov, hipStream_t st, int32_t divisor = 1) {
    if (n < 0 || (n > 0 && (!src || !mmt || !out))) DGC_FAIL(DGC_ERR_INVALID, "dgc_compensate_wire: bad arguments");
    if (divisor < 1 || (divisor > 1 && round_to != DGC_F32))
        DGC_FAIL(DGC_ERR_INVALID, "dgc_compensate_wire_avg: divisor >= 1, and > 1 only for an exchanged (round_to fp32) source");
    if (n == 0) return DGC_OK;
    int mode;
    if (src_dtype == DGC_F16 && round_to == DGC_F32) mode = 1;
    else if (src_dtype == DGC_F32 && round_to == DGC_F16) mode = 2;
    else if (src_dtype == DGC_F32 && round_to == DGC_F32) mode = 0;
    else DGC_FAIL(DGC_ERR_DTYPE, "dgc_compensate_wire: source fp32 (round_to fp32 / fp16) or fp16 (round_to fp32)");
    const int64_t grid = ceil_div(n, (int64_t)kBlock * 4);
    if (grid > 0x7FFFFFFFLL) DGC_FAIL(DGC_ERR_INVALID, "dgc_compensate_wire: n too large");
    const dim3 gd((unsigned)grid), bd(kBlock);
    const float div = (float)divisor;
    with_bool(nesterov, [&](auto NEST) { with_mode<3>(mode, [&](auto MODE) {
        hipLaunchKernelGGL((k_compensate_wire<NEST(), MODE()>), gd, bd, 0, st, src, mmt, out, n, mom, div); }); });
    DGC_LAUNCHED();
    return DGC_OK;
}

// ---- the dense Average as the rank-order sum of an allgather ----
// The reference Average-allreduces every dense tensor (dgc/compression.py:205-206,
// Horovod allreduce_async_(op=Average)); the oracle restates it as Horovod's result on
// the rank-order concatenation: acc = x_0; acc += x_1; ...; acc /= W, every op on a
// tensor of the wire dtype (fp32, or fp16 with fp16_values; bf16 for a bf16 parameter).
// An RCCL / gloo allreduce sums in ITS order, which decides the last bits at W >= 3 —
// so the dense values travel by allgather and are summed here, in rank order. ATen's
// add_ on a 16-bit tensor computes in fp32 and rounds each sum; CPU div_ by the integer
// W is the fp32 TRUE quotient (on 16-bit tensors identical to its reciprocal form: all
// 65536 fp16 / bf16 patterns checked for W = 3..12), rounded to the wire dtype. Rank r's
// n values start at src + r * rank_stride (bytes).
template <int DT>   // DGC_F32 / DGC_F16 / DGC_BF16
__device__ __forceinline__ float wire_at(const char* __restrict__ src, int64_t rank_stride, int r, int64_t e) {
    const char* row = src + (int64_t)r * rank_stride;
    if (DT == DGC_F32) return reinterpret_cast<const float*>(row)[e];
    return h16_to_f32<DT>(reinterpret_cast<const uint16_t*>(row)[e]);
}

template <int DT>
__device__ __forceinline__ float wire_round(float x) {
    if (DT == DGC_F32) return x;
    return round16<DT>(x);
}

template <int DT>
__device__ __forceinline__ float rank_average(const char* __restrict__ src, int64_t rank_stride, int world,
                                              int64_t e, bool average) {
    float acc = wire_at<DT>(src, rank_stride, 0, e);
    for (int r = 1; r < world; ++r) acc = wire_round<DT>(__fadd_rn(acc, wire_at<DT>(src, rank_stride, r, e)));
    if (average) acc = wire_round<DT>(__fdiv_rn(acc, (float)world));
    return acc;
}

// dst[e] = the rank-order sum (/ W for Average) in the wire dtype: the per-tensor
// allreduce (dgc.comm.allreduce_async_). dst may be any rank's row (in place).
template <int DT>
__global__ void __launch_bounds__(kBlock)
k_rank_sum(const char* __restrict__ src, int64_t rank_stride, int world, int64_t n, int average, void* dst) {
    const int64_t e0 = (int64_t)blockIdx.x * kBlock * 4 + threadIdx.x;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t e = e0 + (int64_t)j * kBlock;
        v[j] = e < n ? rank_average<DT>(src, rank_stride, world, e, average != 0) : 0.f;
    }
    // every load above is issued before any store: dst may alias a source row
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t e = e0 + (int64_t)j * kBlock;
        if (e >= n) break;
        if (DT == DGC_F32) static_cast<float*>(dst)[e] = v[j];
        else static_cast<uint16_t*>(dst)[e] = f32_to_h16<DT>(v[j]);
    }
}

// out = compensate(accumulate=False) of the Average of the gathered dense wire values
// (decompress's dense branch, dgc/compression.py:195-198: `tensor.type(vdtype)` widens
// the fp16 wire exactly, then DGCSGDMemory.compensate, dgc/memory.py:64-70).
template <bool NEST, int DT>
__global__ void __launch_bounds__(kBlock)
k_compensate_ranks(const char* __restrict__ src, int64_t rank_stride, int world, float* __restrict__ mmt,
                   float* __restrict__ out, int64_t n, float mom) {
    const int64_t e0 = (int64_t)blockIdx.x * kBlock * 4 + threadIdx.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t e = e0 + (int64_t)j * kBlock;
        if (e >= n) break;
        const float g = rank_average<DT>(src, rank_stride, world, e, true);
        float m = mmt[e], v = 0.f;
        const float o = comp1<NEST, false>(g, m, v, mom);
        mmt[e] = m;
        out[e] = o;
    }
}

static int check_ranks(const void* src, int32_t dtype, int32_t world, int64_t rank_stride, int64_t n,
                       const char* who) {
    if (n < 0 || (n > 0 && !src) || world < 1 || world > 4096)
        DGC_FAIL(DGC_ERR_INVALID, "%s: bad arguments (n %lld, world %d)", who, (long long)n, (int)world);
    if (!wire_ok(dtype, true)) DGC_FAIL(DGC_ERR_DTYPE, "%s: wire dtype", who);
    const int64_t es = vbytes(dtype);
    if (world > 1 && rank_stride < n * es)
        DGC_FAIL(DGC_ERR_INVALID, "%s: rank_stride %lld < %lld bytes of values", who, (long long)rank_stride,
                 (long long)(n * es));
    if ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)rank_stride) & (uintptr_t)(es - 1))
        DGC_FAIL(DGC_ERR_INVALID, "%s: source rows must be aligned to the wire dtype", who);
    if (ceil_div(n, (int64_t)kBlock * 4) > 0x7FFFFFFFLL) DGC_FAIL(DGC_ERR_INVALID, "%s: n too large", who);
    return DGC_OK;
}

int rank_sum(const void* src, int32_t dtype, int32_t world, int64_t rank_stride, int64_t n, int32_t average,
             void* dst, hipStream_t st) {
    DGC_TRY(check_ranks(src, dtype, world, rank_stride, n, "dgc_rank_sum"));
    if (n > 0 && !dst) DGC_FAIL(DGC_ERR_INVALID, "dgc_rank_sum: null destination");
    if (n == 0) return DGC_OK;
    const dim3 gd((unsigned)ceil_div(n, (int64_t)kBlock * 4)), bd(kBlock);
    const char* s = static_cast<const char*>(src);
    with_wire16(dtype, [&](auto DT) {
        hipLaunchKernelGGL((k_rank_sum<DT()>), gd, bd, 0, st, s, rank_stride, world, n, average, dst); });
    DGC_LAUNCHED();
    return DGC_OK;
}

int compensate_ranks(const void* src, int32_t dtype, int32_t world, int64_t rank_stride, float* mmt, float* out,
                     int64_t n, float mom, bool nesterov, hipStream_t st) {
    DGC_TRY(check_ranks(src, dtype, world, rank_stride, n, "dgc_compensate_ranks"));
    if (dtype == DGC_BF16) DGC_FAIL(DGC_ERR_DTYPE, "dgc_compensate_ranks: fp32 parameters take an fp32 or fp16 wire");
    if (n > 0 && (!mmt || !out)) DGC_FAIL(DGC_ERR_INVALID, "dgc_compensate_ranks: null mmt / out");
    if (n == 0) return DGC_OK;
    const dim3 gd((unsigned)ceil_div(n, (int64_t)kBlock * 4)), bd(kBlock);
    const char* s = static_cast<const char*>(src);
    with_bool(nesterov, [&](auto NEST) { with_vd(dtype, [&](auto DT) {   // bf16 was refused above
        hipLaunchKernelGGL((k_compensate_ranks<NEST(), DT()>), gd, bd, 0, st, s, rank_stride, world, mmt, out, n, mom); }); });
    DGC_LAUNCHED();
    return DGC_OK;
}

// K1 with the gradient clipped as it is loaded (ca.tab points at this tensor's coefficient).
int compensate_clip(const float* grad, float* mmt, float* vec, float* out, int64_t n, float momentum,
                    bool nesterov, bool accumulate, float* samples, int64_t s_start, int64_t s_stride,
                    int64_t s_count, int32_t clip_kind, ClipArg ca, hipStream_t st) {
    if (n < 0) DGC_FAIL(DGC_ERR_INVALID, "dgc_compensate: n < 0");
    DGC_TRY(check_clip("dgc_compensate", clip_kind, ca.tab));
    if (n == 0) return DGC_OK;
    if (!grad || !mmt) DGC_FAIL(DGC_ERR_INVALID, "dgc_compensate: null grad/mmt");
    if (accumulate && !vec) DGC_FAIL(DGC_ERR_INVALID, "dgc_compensate: accumulate needs vec");
    if (accumulate && out && out != vec)
        DGC_FAIL(DGC_ERR_INVALID, "dgc_compensate: accumulate writes vec (out must be NULL or vec)");
    if (!accumulate && !out) DGC_FAIL(DGC_ERR_INVALID, "dgc_compensate: dense branch needs out");
    SampleSpec sp{nullptr, 0, 1, 0, 1.0, 1.0f};
    if (samples) {
        if (!accumulate) DGC_FAIL(DGC_ERR_INVALID, "dgc_compensate: sampling needs accumulate=1");
        if (s_stride < 1 || s_start < 0 || s_start >= n)
            DGC_FAIL(DGC_ERR_INVALID, "dgc_compensate: bad sample start/stride");
        if (s_count != ceil_div(n - s_start, s_stride))
            DGC_FAIL(DGC_ERR_INVALID, "dgc_compensate: num_samples must be ceil((n-start)/stride)");
        sp = SampleSpec{samples, s_start, s_stride, s_count, 1.0 / (double)s_stride, 1.0f / (float)s_stride};
        if (s_stride < 4) {
            // tiny strides (sample_ratio >= 0.25): unfused, samples read back after the pass
            DGC_TRY(compensate_clip(grad, mmt, vec, out, n, momentum, nesterov, accumulate, nullptr, 0,
                                    1, 0, clip_kind, ca, st));
            const int grid = grid_for(s_count);
            hipLaunchKernelGGL(k_sample_strided, dim3(grid), dim3(kBlock), 0, st, vec, s_start,
                               s_stride, s_count, samples);
            DGC_LAUNCHED();
            return DGC_OK;
        }
    }
    return with_bool(nesterov, [&](auto NEST) { return with_bool(accumulate, [&](auto ACC) {
        return with_clip(clip_kind, [&](auto CLIP) {
            return launch_comp<NEST(), ACC(), CLIP()>(grad, mmt, vec, out, n, momentum, sp, ca, st); }); }); });
}

int compensate(const float* grad, float* mmt, float* vec, float* out, int64_t n, float momentum,
               bool nesterov, bool accumulate, float* samples, int64_t s_start, int64_t s_stride,
               int64_t s_count, hipStream_t st) {
    return compensate_clip(grad, mmt, vec, out, n, momentum, nesterov, accumulate, samples, s_start, s_stride,
                           s_count, DGC_CLIP_NONE, ClipArg{nullptr, 0.f}, st);
}

}  // namespace dgc

// Ceiling probe for K1's access mix: three 16-B non-temporal reads and two 16-B
// non-temporal writes per float4, one-shot 256-thread blocks — K1's memory shape
// with no arithmetic to speak of. The bench runs it on its own buffers after the
// timed steps to measure what the box it landed on streams (boxes differ by ~10 %).
__global__ void __launch_bounds__(dgc::kBlock)
k_probe_3r2w(const float4* __restrict__ a, const float4* __restrict__ b, const float4* __restrict__ c,
             float4* __restrict__ d, float4* __restrict__ e, int64_t n4) {
    const int64_t v = (int64_t)blockIdx.x * dgc::kBlock + threadIdx.x;
    if (v >= n4) return;
    const float4 x = dgc::ld_nt(a + v), y = dgc::ld_nt(b + v), z = dgc::ld_nt(c + v);
    dgc::st_nt(d + v, make_float4(x.x + z.x, x.y + z.y, x.z + z.z, x.w + z.w));
    dgc::st_nt(e + v, make_float4(y.x + z.x, y.y + z.y, y.z + z.z, y.w + z.w));
}

extern "C" int dgc_hbm_probe(const float* a, const float* b, const float* c, float* d, float* e, int64_t n,
                             void* stream) {
    if (!a || !b || !c || !d || !e || n < 4) DGC_FAIL(DGC_ERR_INVALID, "dgc_hbm_probe: bad arguments");
    if (!dgc::aligned16(a) || !dgc::aligned16(b) || !dgc::aligned16(c) || !dgc::aligned16(d) || !dgc::aligned16(e))
        DGC_FAIL(DGC_ERR_INVALID, "dgc_hbm_probe: buffers must be 16-B aligned");
    const int64_t n4 = n / 4;
    if (dgc::ceil_div(n4, (int64_t)dgc::kBlock) > 0x7FFFFFFFLL) DGC_FAIL(DGC_ERR_INVALID, "dgc_hbm_probe: n too large");
    hipLaunchKernelGGL(k_probe_3r2w, dim3((unsigned)dgc::ceil_div(n4, (int64_t)dgc::kBlock)), dim3(dgc::kBlock), 0,
                       static_cast<hipStream_t>(stream), reinterpret_cast<const float4*>(a),
                       reinterpret_cast<const float4*>(b), reinterpret_cast<const float4*>(c),
                       reinterpret_cast<float4*>(d), reinterpret_cast<float4*>(e), n4);
    DGC_LAUNCHED();
    return DGC_OK;
}

extern "C" int dgc_compensate(const float* grad, float* mmt, float* vec, float* out, int64_t n,
                              float momentum, int32_t nesterov, int32_t accumulate, float* samples,
                              int64_t sample_start, int64_t sample_stride, int64_t num_samples,
                              void* stream) {
    return dgc::compensate(grad, mmt, vec, out, n, momentum, nesterov != 0, accumulate != 0, samples,
                           sample_start, sample_stride, num_samples,
                           static_cast<hipStream_t>(stream));
}

extern "C" int dgc_gather_cast(const float* const* srcs, const int64_t* numels, const int64_t* offsets,
                               int32_t count, void* dst, int32_t dst_dtype, void* stream) {
    return dgc::gather_cast(srcs, numels, offsets, count, dst, dst_dtype, static_cast<hipStream_t>(stream));
}

extern "C" int dgc_compensate_multi(const float* const* srcs, const int64_t* numels, const int64_t* offsets,
                                    int32_t count, int32_t round_to, float* mmt, float* out, float momentum,
                                    int32_t nesterov, void* stream) {
    return dgc::compensate_multi(srcs, numels, offsets, count, round_to, mmt, out, momentum, nesterov != 0,
                                 DGC_CLIP_NONE, dgc::ClipArg{nullptr, 0.f}, static_cast<hipStream_t>(stream));
}

extern "C" int dgc_compensate_multi_clip(const float* const* srcs, const int64_t* numels, const int64_t* offsets,
                                         int32_t count, int32_t round_to, float* mmt, float* out, float momentum,
                                         int32_t nesterov, int32_t clip_kind, const float* clip, float clip_value,
                                         void* stream) {
    return dgc::compensate_multi(srcs, numels, offsets, count, round_to, mmt, out, momentum, nesterov != 0,
                                 clip_kind, dgc::ClipArg{clip, clip_value}, static_cast<hipStream_t>(stream));
}

extern "C" int dgc_compensate_clip(const float* grad, float* mmt, float* vec, float* out, int64_t n, float momentum,
                                   int32_t nesterov, int32_t accumulate, float* samples, int64_t sample_start,
                                   int64_t sample_stride, int64_t num_samples, int32_t clip_kind, const float* clip,
                                   float clip_value, void* stream) {
    return dgc::compensate_clip(grad, mmt, vec, out, n, momentum, nesterov != 0, accumulate != 0, samples,
                                sample_start, sample_stride, num_samples, clip_kind, dgc::ClipArg{clip, clip_value},
                                static_cast<hipStream_t>(stream));
}

extern "C" int dgc_compensate_wire(const void* src, int32_t src_dtype, int32_t round_to, float* mmt, float* out,
                                   int64_t n, float momentum, int32_t nesterov, void* stream) {
    return dgc::compensate_wire(src, src_dtype, round_to, mmt, out, n, momentum, nesterov != 0,
                                static_cast<hipStream_t>(stream));
}

extern "C" int dgc_compensate_wire_avg(const void* src, int32_t src_dtype, int32_t world, float* mmt, float* out,
                                       int64_t n, float momentum, int32_t nesterov, void* stream) {
    return dgc::compensate_wire(src, src_dtype, DGC_F32, mmt, out, n, momentum, nesterov != 0,
                                static_cast<hipStream_t>(stream), world);
}

extern "C" int dgc_rank_sum(const void* src, int32_t dtype, int32_t world, int64_t rank_stride, int64_t n,
                            int32_t average, void* dst, void* stream) {
    return dgc::rank_sum(src, dtype, world, rank_stride, n, average, dst, static_cast<hipStream_t>(stream));
}

extern "C" int dgc_compensate_ranks(const void* src, int32_t src_dtype, int32_t world, int64_t rank_stride,
                                    float* mmt, float* out, int64_t n, float momentum, int32_t nesterov,
                                    void* stream) {
    return dgc::compensate_ranks(src, src_dtype, world, rank_stride, mmt, out, n, momentum, nesterov != 0,
                                 static_cast<hipStream_t>(stream));
}

extern "C" int dgc_sample_strided(const float* vec, int64_t n, int64_t start, int64_t stride,
                                  float* samples, int64_t num_samples, void* stream) {
    if (!vec || !samples || stride < 1 || start < 0 || (n > 0 && start >= n))
        DGC_FAIL(DGC_ERR_INVALID, "dgc_sample_strided: bad arguments");
    if (num_samples != dgc::ceil_div(n - start, stride))
        DGC_FAIL(DGC_ERR_INVALID, "dgc_sample_strided: num_samples must be ceil((n-start)/stride)");
    if (num_samples == 0) return DGC_OK;
    hipLaunchKernelGGL(dgc::k_sample_strided, dim3(dgc::grid_for(num_samples)), dim3(dgc::kBlock), 0,
                       static_cast<hipStream_t>(stream), vec, start, stride, num_samples, samples);
    DGC_LAUNCHED();
    return DGC_OK;
}

extern "C" int dgc_sample_gather(const float* vec, const int64_t* sample_indices, int64_t num_samples,
                                 float* samples, void* stream) {
    if (!vec || !sample_indices || !samples || num_samples < 0)
        DGC_FAIL(DGC_ERR_INVALID, "dgc_sample_gather: bad arguments");
    if (num_samples == 0) return DGC_OK;
    hipLaunchKernelGGL(dgc::k_sample_gather, dim3(dgc::grid_for(num_samples)), dim3(dgc::kBlock), 0,
                       static_cast<hipStream_t>(stream), vec, sample_indices, num_samples, samples);
    DGC_LAUNCHED();
    return DGC_OK;
}

extern "C" int dgc_mask_indices(float* mmt, float* vec, int64_t n, const void* indices, int32_t idtype,
                                int64_t count, int32_t* bad_flag, void* stream) {
    if (!vec || (count > 0 && !indices) || !bad_flag)
        DGC_FAIL(DGC_ERR_INVALID, "dgc_mask_indices: null argument");
    if (!dgc::index_ok(idtype)) DGC_FAIL(DGC_ERR_DTYPE, "dgc_mask_indices: index dtype");
    if (count <= 0) return DGC_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int grid = dgc::grid_for(count);
    dgc::with_id(idtype, [&](auto ID) {
        using I = dgc::idx_t<decltype(ID)>;
        hipLaunchKernelGGL(dgc::k_mask<I>, dim3(grid), dim3(dgc::kBlock), 0, s, mmt, vec, static_cast<const I*>(indices),
                           count, n, bad_flag); });
    DGC_LAUNCHED();
    return DGC_OK;
}
