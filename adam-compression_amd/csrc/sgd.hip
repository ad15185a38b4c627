// K7: DGCSGD.step fused — weight-decay momentum and the parameter update in one
// streaming pass over every parameter of a group (dgc/optim/sgd.py:42-68).
//
// DGC applies the gradient's momentum in DGCSGDMemory.compensate, so the optimizer
// keeps momentum for the weight-decay term only. Per element, with the reference's
// torch-CPU rounding (probed: Tensor * python-float = fl(x * fl32(s)); add(b, alpha)
// = fmadd(b, alpha, a), ONE rounding, in both the vector and the scalar loops):
//
//   wd != 0:  d = p * wd                                  (mul)
//             mom != 0:  first step:  buf = d             (momentum_buffer = d_p)
//                        else:        buf = buf * mom     (mul_)
//                                     buf = fma(d, 1 - dampening, buf)   (add_(alpha))
//                        nesterov:    d = fma(buf, mom, d)               (add(alpha))
//                        else:        d = buf
//             d = d + g                                   (add)
//   wd == 0:  d = g
//   p = fma(d, -lr, p)                                    (add_(alpha=-lr))
//
// HBM: read p, g (+ buf), write p (+ buf): 12 or 20 B per element. One launch covers
// up to kSgdMaxTensors tensors (a block table in the kernel arguments, like a
// multi-tensor apply); each block streams 16-B vectors of one tensor.
//
// The entry points check the WHOLE table before the first chunk is launched: a refusal
// leaves every tensor untouched. An entry with numels[i] == 0 may carry null pointers (a
// zero-element device tensor has a null data pointer): it gets no block, so none of its
// pointers is read, and the step is the no-op the reference's is. With n > 0 a null
// params[i] / grads[i] (or bufs[i], when a momentum buffer is in use) is refused.
#include "dispatch.hpp"
#include "payload.hpp"

namespace dgc {

constexpr int kSgdMaxTensors = 48;
constexpr int kSgdPerBlock = kBlock * 4 * 4;   // 4 float4 per lane per block

struct SgdTable {
    float* p[kSgdMaxTensors];
    const float* g[kSgdMaxTensors];
    float* buf[kSgdMaxTensors];
    int64_t n[kSgdMaxTensors];
    int32_t block0[kSgdMaxTensors + 1];   // first block of each tensor; block0[count] = grid
    int32_t first[kSgdMaxTensors];        // momentum buffer created on this step
    int32_t count;
};

struct SgdHyper {
    float wd, mom, damp_alpha, neg_lr;
    int32_t nesterov;
};

// The table of dgc_sgd_step / dgc_sgd_step16, every entry, before anything is launched.
static int sgd_check_table(const char* who, const void* const* params, const void* const* grads,
                           const void* const* bufs, const int64_t* numels, int32_t count, bool mom,
                           int64_t per_block) {
    int64_t blocks = 0;   // of the chunk (one launch) tensor i is in
    for (int32_t i = 0; i < count; ++i) {
        if (numels[i] < 0) DGC_FAIL(DGC_ERR_INVALID, "%s: tensor %d: n < 0", who, i);
        if (numels[i] > 0 && (!params[i] || !grads[i] || (mom && !bufs[i])))
            DGC_FAIL(DGC_ERR_INVALID, "%s: tensor %d: null pointer", who, i);
        if (i % kSgdMaxTensors == 0) blocks = 0;
        blocks += ceil_div(numels[i], per_block);
        if (blocks > 0x7FFFFFFF) DGC_FAIL(DGC_ERR_INVALID, "%s: too many elements in one group", who);
    }
    return DGC_OK;
}

template <bool WD, bool MOM>
__device__ __forceinline__ float sgd1(float p, float g, float& b, bool first, const SgdHyper& h) {
    float d = g;
    if (WD) {
        d = __fmul_rn(p, h.wd);
        if (MOM) {
            if (first) {
                b = d;
            } else {
                b = __fmul_rn(b, h.mom);
                b = __fmaf_rn(d, h.damp_alpha, b);
            }
            d = h.nesterov ? __fmaf_rn(b, h.mom, d) : b;
        }
        d = __fadd_rn(d, g);
    }
    return __fmaf_rn(d, h.neg_lr, p);
}

template <bool WD, bool MOM>
__global__ void __launch_bounds__(kBlock) k_sgd(SgdTable t, SgdHyper h) {
    // the tensor of this block: block0 is ascending, <= 48 entries (scalar search)
    int ti = 0;
    while (ti + 1 < t.count && (int)blockIdx.x >= t.block0[ti + 1]) ++ti;
    float* __restrict__ p = t.p[ti];
    const float* __restrict__ g = t.g[ti];
    float* __restrict__ buf = t.buf[ti];
    const int64_t n = t.n[ti];
    const bool first = t.first[ti] != 0;
    const int64_t base = (int64_t)(blockIdx.x - t.block0[ti]) * kSgdPerBlock;
    const bool vec = aligned16(p) && aligned16(g) && (!MOM || aligned16(buf));
    if (vec && base + kSgdPerBlock <= n) {
        float4 pv[4], gv[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = base + (int64_t)(u * kBlock + threadIdx.x) * 4;
            pv[u] = ld_nt(reinterpret_cast<const float4*>(p + i));
            gv[u] = ld_nt(reinterpret_cast<const float4*>(g + i));
            if (MOM && !first) bv[u] = ld_nt(reinterpret_cast<const float4*>(buf + i));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = base + (int64_t)(u * kBlock + threadIdx.x) * 4;
            float4 o;
            o.x = sgd1<WD, MOM>(pv[u].x, gv[u].x, bv[u].x, first, h);
            o.y = sgd1<WD, MOM>(pv[u].y, gv[u].y, bv[u].y, first, h);
            o.z = sgd1<WD, MOM>(pv[u].z, gv[u].z, bv[u].z, first, h);
            o.w = sgd1<WD, MOM>(pv[u].w, gv[u].w, bv[u].w, first, h);
            st_nt(reinterpret_cast<float4*>(p + i), o);
            if (MOM) st_nt(reinterpret_cast<float4*>(buf + i), bv[u]);
        }
        return;
    }
    const int64_t end = base + kSgdPerBlock < n ? base + kSgdPerBlock : n;
    for (int64_t i = base + threadIdx.x; i < end; i += kBlock) {
        float b = MOM && !first ? buf[i] : 0.f;
        p[i] = sgd1<WD, MOM>(p[i], g[i], b, first, h);
        if (MOM) buf[i] = b;
    }
}

// K7-16: DGCSGD.step on bf16 / fp16 parameters (DT): the same op sequence, every ATen
// op rounding to the dtype (it computes in fp32). `x.add(y, alpha)` on a 16-bit CPU
// tensor rounds alpha to the dtype; its vectorised body (the first n - n % 32 elements)
// rounds fl32(x + y * alpha) once (the product of two 16-bit values is exact in fp32),
// its scalar tail rounds the product to the dtype first (oracle.dgcsgd_step16, pinned
// to the reference's run in tests/golden/sgd16.*). 6 or 10 B per element.
constexpr int kSgd16PerThread = 4;
constexpr int kSgd16PerBlock = kBlock * kSgd16PerThread;

struct Sgd16Table {
    uint16_t* p[kSgdMaxTensors];
    const uint16_t* g[kSgdMaxTensors];
    uint16_t* buf[kSgdMaxTensors];
    int64_t n[kSgdMaxTensors];
    int32_t block0[kSgdMaxTensors + 1];
    int32_t first[kSgdMaxTensors];
    int32_t count;
};

template <int DT>
__device__ __forceinline__ float add_alpha16(float a, float b, float al, bool tail) {
    const float prod = __fmul_rn(b, al);
    return round16<DT>(__fadd_rn(a, tail ? round16<DT>(prod) : prod));
}

template <int DT, bool WD, bool MOM>
__global__ void __launch_bounds__(kBlock) k_sgd16(Sgd16Table t, SgdHyper h) {
    int ti = 0;
    while (ti + 1 < t.count && (int)blockIdx.x >= t.block0[ti + 1]) ++ti;
    uint16_t* __restrict__ p = t.p[ti];
    const uint16_t* __restrict__ g = t.g[ti];
    uint16_t* __restrict__ buf = t.buf[ti];
    const int64_t n = t.n[ti];
    const int64_t body = n - n % 32;
    const bool first = t.first[ti] != 0;
    // alphas rounded to the dtype (the CPU kernels' scalar_t alpha)
    const float a_damp = round16<DT>(h.damp_alpha), a_mom = round16<DT>(h.mom), a_lr = round16<DT>(h.neg_lr);
    const int64_t base = (int64_t)(blockIdx.x - t.block0[ti]) * kSgd16PerBlock;
#pragma unroll
    for (int u = 0; u < kSgd16PerThread; ++u) {
        const int64_t i = base + (int64_t)u * kBlock + threadIdx.x;
        if (i >= n) break;
        const bool tail = i >= body;
        const float pv = h16_to_f32<DT>(p[i]), gv = h16_to_f32<DT>(g[i]);
        float d = gv;
        if (WD) {
            d = round16<DT>(__fmul_rn(pv, h.wd));                        // weight_decay * p.data
            if (MOM) {
                float b;
                if (first) {
                    b = d;                                               // buf = d_p
                } else {
                    b = round16<DT>(__fmul_rn(h16_to_f32<DT>(buf[i]), h.mom));   // buf.mul_(momentum)
                    b = add_alpha16<DT>(b, d, a_damp, tail);             // .add_(d_p, alpha=1 - dampening)
                }
                buf[i] = f32_to_h16<DT>(b);
                d = h.nesterov ? add_alpha16<DT>(d, b, a_mom, tail) : b;
            }
            d = round16<DT>(__fadd_rn(d, gv));                           // d_p.add(p.grad)
        }
        p[i] = f32_to_h16<DT>(add_alpha16<DT>(pv, d, a_lr, tail));       // p.add_(d_p, alpha=-lr)
    }
}

}  // namespace dgc

extern "C" int dgc_sgd_step16(void* const* params, const void* const* grads, void* const* bufs,
                              const int64_t* numels, const int32_t* first, int32_t count, float lr, float momentum,
                              float dampening, float weight_decay, int32_t nesterov, int32_t dtype, void* stream) {
    using namespace dgc;
    if (count < 0 || (count > 0 && (!params || !grads || !numels)))
        DGC_FAIL(DGC_ERR_INVALID, "dgc_sgd_step16: null tensor table");
    if (!is16(dtype)) DGC_FAIL(DGC_ERR_DTYPE, "dgc_sgd_step16: dtype must be bf16 or fp16");
    const bool wd = weight_decay != 0.f, mom = wd && momentum != 0.f;
    if (count > 0 && mom && (!bufs || !first)) DGC_FAIL(DGC_ERR_INVALID, "dgc_sgd_step16: momentum needs buffers");
    DGC_TRY(sgd_check_table("dgc_sgd_step16", params, grads, bufs, numels, count, mom, kSgd16PerBlock));
    SgdHyper h{weight_decay, momentum, 1.f - dampening, -lr, nesterov};
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int32_t c0 = 0; c0 < count; c0 += kSgdMaxTensors) {
        Sgd16Table t{};
        int64_t blocks = 0;
        for (int32_t j = 0; j < kSgdMaxTensors && c0 + j < count; ++j) {
            const int32_t i = c0 + j;
            t.p[t.count] = static_cast<uint16_t*>(params[i]);
            t.g[t.count] = static_cast<const uint16_t*>(grads[i]);
            t.buf[t.count] = mom ? static_cast<uint16_t*>(bufs[i]) : nullptr;
            t.n[t.count] = numels[i];
            t.first[t.count] = mom ? first[i] : 0;
            t.block0[t.count] = (int32_t)blocks;
            blocks += ceil_div(numels[i], (int64_t)kSgd16PerBlock);
            t.count++;
        }
        t.block0[t.count] = (int32_t)blocks;
        if (blocks == 0) continue;
        const dim3 gd((unsigned)blocks), bd(kBlock);
        // momentum only with weight decay (mom implies wd): three kernels per dtype, not four
        with_h16(dtype, [&](auto DT) { with_bool(wd, [&](auto WD) { with_bool(mom, [&](auto MOM) {
            hipLaunchKernelGGL((k_sgd16<DT(), WD(), WD() && MOM()>), gd, bd, 0, s, t, h); }); }); });
        DGC_LAUNCHED();
    }
    return DGC_OK;
}

extern "C" int dgc_sgd_step(float* const* params, const float* const* grads, float* const* bufs,
                            const int64_t* numels, const int32_t* first, int32_t count, float lr, float momentum,
                            float dampening, float weight_decay, int32_t nesterov, void* stream) {
    using namespace dgc;
    if (count < 0 || (count > 0 && (!params || !grads || !numels)))
        DGC_FAIL(DGC_ERR_INVALID, "dgc_sgd_step: null tensor table");
    const bool wd = weight_decay != 0.f, mom = wd && momentum != 0.f;
    if (count > 0 && mom && (!bufs || !first)) DGC_FAIL(DGC_ERR_INVALID, "dgc_sgd_step: momentum needs buffers");
    DGC_TRY(sgd_check_table("dgc_sgd_step", reinterpret_cast<const void* const*>(params),
                            reinterpret_cast<const void* const*>(grads),
                            reinterpret_cast<const void* const*>(bufs), numels, count, mom, kSgdPerBlock));
    SgdHyper h{weight_decay, momentum, 1.f - dampening, -lr, nesterov};
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int32_t c0 = 0; c0 < count; c0 += kSgdMaxTensors) {
        SgdTable t{};
        int64_t blocks = 0;
        for (int32_t j = 0; j < kSgdMaxTensors && c0 + j < count; ++j) {
            const int32_t i = c0 + j;
            t.p[t.count] = params[i];
            t.g[t.count] = grads[i];
            t.buf[t.count] = mom ? bufs[i] : nullptr;
            t.n[t.count] = numels[i];
            t.first[t.count] = mom ? first[i] : 0;
            t.block0[t.count] = (int32_t)blocks;
            blocks += ceil_div(numels[i], (int64_t)kSgdPerBlock);
            t.count++;
        }
        t.block0[t.count] = (int32_t)blocks;
        if (blocks == 0) continue;
        with_bool(wd, [&](auto WD) { with_bool(mom, [&](auto MOM) {   // mom implies wd: three kernels
            hipLaunchKernelGGL((k_sgd<WD(), WD() && MOM()>), dim3((unsigned)blocks), dim3(kBlock), 0, s, t, h); }); });
        DGC_LAUNCHED();
    }
    return DGC_OK;
}

// ---------------------------------------------------------------- sparse step
// dgc_apply_packed: DGCSGD.step on the flat bucket without a dense gradient. `acc` holds
// the decompressed gradient (dgc_scatter_packed of the gathered payload onto +0.0): +0.0
// everywhere but at <= W * k gathered indices. The kernels walk the payload's entries
// (all W runs) instead of the N elements; an entry takes its slot with a 32-bit atomic
// exchange against +0.0 (relaxed, agent scope: an integer swap, never a float add), so
// exactly one entry per distinct index gets the sum — whichever wins computes the same
// result — duplicates across ranks get +0.0, and acc is +0.0 again when the walk ends.
//
// An entry whose slot holds +0.0 (all bits zero) is skipped, which is exact:
//   wd == 0:  the reference computes fma(+0, -lr, p) = p + (-0) = p for every p, +-0
//             included (lr >= 0, so -lr carries the sign bit even at lr = 0);
//   wd != 0:  the dense pass below already computed the g = +0 result.
// -0.0 and NaN have nonzero bits and are applied.
//
//   wd == 0:  k_apply_entries<APPLY>: p[i] = fma(g, -lr, p[i]), O(W k) in all.
//   wd != 0:  k_apply_entries<STASH>: stash[q] = p[i] (entry q = rank * capacity + slot;
//               duplicates store the same value);
//             k_sgd_zero_grad: K7 with g = +0.0 and no gradient load, 16 (8 without
//               momentum) B per element against K7's 20 (12). The d + 0 add stays: with
//               p = -0.0, wd * p = -0 and the reference's d.add(grad) makes it +0;
//             k_apply_entries<FIXUP>: the winner recomputes its element from stash[q] and
//               the new buf[i] (which does not depend on g) with g.
// The walk reads the header counts as the scatter does (RunSrc::get_raw: clamped to
// [0, capacity]), so it visits exactly the entries the scatter summed; an index outside
// [0, n) is skipped before any access. The scatter flagged both.
namespace dgc {

enum { kApply = 0, kApplyStash = 1, kApplyFixup = 2 };

struct ApplySrc {
    const char* payload;
    int64_t stride, ioff, capacity;
};

// The fix-up of one gathered element of a weight-decay group: the element recomputed from its
// stashed old value and the new buf (which does not depend on g) with its gradient g.
__device__ __forceinline__ float sgd_fixup(float p_old, float g, float b, bool mom, const SgdHyper& h) {
    float d = __fmul_rn(p_old, h.wd);
    if (mom) d = h.nesterov ? __fmaf_rn(b, h.mom, d) : b;
    d = __fadd_rn(d, g);
    return __fmaf_rn(d, h.neg_lr, p_old);
}

template <int ID, int MODE, bool MOM>
__global__ void __launch_bounds__(kBlock)
k_apply_entries(ApplySrc src, float* __restrict__ acc, float* __restrict__ p, const float* __restrict__ buf,
                float* __restrict__ stash, int64_t n, SgdHyper h) {
    const int r = (int)blockIdx.y;
    const char* base = src.payload + (int64_t)r * src.stride;
    const long long cnt = payload_count(base, src.capacity);
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < cnt; e += (long long)gridDim.x * kBlock) {
        const long long i = load_wire_idx<ID>(base + src.ioff, e);
        if (i < 0 || i >= n) continue;
        const int64_t q = (int64_t)r * src.capacity + e;
        if (MODE == kApplyStash) {
            stash[q] = p[i];
            continue;
        }
        const uint32_t gb = __hip_atomic_exchange(reinterpret_cast<uint32_t*>(acc + i), 0u, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_AGENT);
        if (gb == 0u) continue;   // +0.0: a duplicate's second visit, or a sum of +0.0 (see above)
        const float g = __uint_as_float(gb);
        if (MODE == kApply) {
            p[i] = __fmaf_rn(g, h.neg_lr, p[i]);
        } else {
            p[i] = sgd_fixup(stash[q], g, MOM ? buf[i] : 0.f, MOM, h);
        }
    }
}

// K7 with weight decay on one tensor and g = +0.0: k_sgd's load and store shape without
// the gradient stream.
template <bool MOM>
__device__ __forceinline__ void sgd_zero_grad_block(float* __restrict__ p, float* __restrict__ buf, int64_t n,
                                                    bool first, const SgdHyper& h, int64_t block) {
    const int64_t base = block * kSgdPerBlock;
    const bool vec = aligned16(p) && (!MOM || aligned16(buf));
    if (vec && base + kSgdPerBlock <= n) {
        float4 pv[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = base + (int64_t)(u * kBlock + threadIdx.x) * 4;
            pv[u] = ld_nt(reinterpret_cast<const float4*>(p + i));
            if (MOM && !first) bv[u] = ld_nt(reinterpret_cast<const float4*>(buf + i));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = base + (int64_t)(u * kBlock + threadIdx.x) * 4;
            float4 o;
            o.x = sgd1<true, MOM>(pv[u].x, 0.f, bv[u].x, first, h);
            o.y = sgd1<true, MOM>(pv[u].y, 0.f, bv[u].y, first, h);
            o.z = sgd1<true, MOM>(pv[u].z, 0.f, bv[u].z, first, h);
            o.w = sgd1<true, MOM>(pv[u].w, 0.f, bv[u].w, first, h);
            st_nt(reinterpret_cast<float4*>(p + i), o);
            if (MOM) st_nt(reinterpret_cast<float4*>(buf + i), bv[u]);
        }
        return;
    }
    const int64_t end = base + kSgdPerBlock < n ? base + kSgdPerBlock : n;
    for (int64_t i = base + threadIdx.x; i < end; i += kBlock) {
        float b = MOM && !first ? buf[i] : 0.f;
        p[i] = sgd1<true, MOM>(p[i], 0.f, b, first, h);
        if (MOM) buf[i] = b;
    }
}

template <bool MOM>
__global__ void __launch_bounds__(kBlock)
k_sgd_zero_grad(float* __restrict__ p, float* __restrict__ buf, int64_t n, int32_t first_i, SgdHyper h) {
    sgd_zero_grad_block<MOM>(p, buf, n, first_i != 0, h, (int64_t)blockIdx.x);
}

static size_t apply_workspace(int32_t world, int64_t capacity) {
    if (world < 1 || capacity < 0) return 0;
    const int64_t slots = (int64_t)world * capacity;
    return align_up((size_t)(slots > 0 ? slots : 1) * sizeof(float), 256);
}

template <int ID>
static int apply_packed(const ApplySrc& src, int32_t world, float* acc, float* p, float* buf, int32_t first,
                        int64_t n, const SgdHyper& h, bool mom, float* stash, hipStream_t s) {
    const dim3 grid((unsigned)grid_for(src.capacity, kBlock, kMaxGrid / 2), (unsigned)world), block(kBlock);
    const bool entries = src.capacity > 0;
    if (h.wd == 0.f) {
        if (entries) {
            hipLaunchKernelGGL((k_apply_entries<ID, kApply, false>), grid, block, 0, s, src, acc, p, nullptr, nullptr, n,
                               h);
            DGC_LAUNCHED();
        }
        return DGC_OK;
    }
    if (entries) {
        hipLaunchKernelGGL((k_apply_entries<ID, kApplyStash, false>), grid, block, 0, s, src, acc, p, nullptr, stash, n,
                           h);
        DGC_LAUNCHED();
    }
    const dim3 dense((unsigned)ceil_div(n, (int64_t)kSgdPerBlock));
    if (!mom) {   // the kernels without momentum take no buffer
        buf = nullptr;
        first = 0;
    }
    return with_bool(mom, [&](auto MOM) -> int {
        hipLaunchKernelGGL(k_sgd_zero_grad<MOM()>, dense, block, 0, s, p, buf, n, first, h);
        DGC_LAUNCHED();
        if (entries) {
            hipLaunchKernelGGL((k_apply_entries<ID, kApplyFixup, MOM()>), grid, block, 0, s, src, acc, p, buf, stash, n, h);
            DGC_LAUNCHED();
        }
        return DGC_OK; });
}

}  // namespace dgc

extern "C" size_t dgc_apply_packed_workspace(int32_t world, int64_t capacity) {
    return dgc::apply_workspace(world, capacity);
}

extern "C" int dgc_apply_packed(const void* payload, int32_t world, int64_t rank_stride, int64_t capacity,
                                int32_t vdtype, int32_t idtype, float* acc, float* param, float* buf, int32_t first,
                                int64_t n, float lr, float momentum, float dampening, float weight_decay,
                                int32_t nesterov, void* ws, size_t ws_bytes, void* stream) {
    using namespace dgc;
    if (!payload || !acc || !param) DGC_FAIL(DGC_ERR_INVALID, "dgc_apply_packed: null payload, acc or param");
    if (world < 1 || world > 64) DGC_FAIL(DGC_ERR_INVALID, "dgc_apply_packed: world %d outside 1..64", world);
    DGC_TRY(check_wire("dgc_apply_packed", vdtype, idtype));
    if (capacity < 0 || n < 1) DGC_FAIL(DGC_ERR_INVALID, "dgc_apply_packed: capacity < 0 or n < 1");
    if (ceil_div(n, (int64_t)kSgdPerBlock) > 0x7FFFFFFFLL) DGC_FAIL(DGC_ERR_INVALID, "dgc_apply_packed: n too large");
    int64_t ioff = 0;
    const int64_t min_stride = payload_layout(capacity, vdtype, idtype, nullptr, &ioff);
    DGC_TRY(check_stride("dgc_apply_packed", rank_stride, min_stride));
    // lr >= 0 (a NaN fails too): the skip of a +0.0 slot needs -lr to carry the sign bit
    if (!(lr >= 0.f)) DGC_FAIL(DGC_ERR_INVALID, "dgc_apply_packed: lr must be >= 0");
    const bool wd = weight_decay != 0.f, mom = wd && momentum != 0.f;
    if (mom && !buf) DGC_FAIL(DGC_ERR_INVALID, "dgc_apply_packed: weight-decay momentum needs buf");
    const size_t need = apply_workspace(world, capacity);
    if (wd && (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 3)))
        DGC_FAIL(DGC_ERR_WORKSPACE, "dgc_apply_packed: weight decay needs a workspace of %zu bytes, 4-B aligned", need);
    const SgdHyper h{weight_decay, momentum, 1.f - dampening, -lr, nesterov};
    const ApplySrc src{static_cast<const char*>(payload), rank_stride, ioff, capacity};
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* stash = static_cast<float*>(ws);
    return with_id(idtype, [&](auto ID) { return apply_packed<ID()>(src, world, acc, param, buf, first, n, h, mom, stash, s); });
}

// ---------------------------------------------------------------- sparse step, multi-tensor
// dgc_apply_packed_multi: the same step for the T tensors of a batch, side by side in one
// flat index space, each with its parameter group's hyper-parameters (<= kApplyMaxGroups
// sets in the kernel arguments). The rows (dgc_apply_row) live in device memory the caller
// keeps: an entry finds its row by binary search over the offsets, a block of the dense
// pass by binary search over block0. Three launches at most, whatever T is:
//   k_apply_entries_multi<kApplyStash>  stash[q] = param[t][i - offset[t]] at the entries
//                                       of weight-decay groups (skipped when there is none);
//   k_sgd_zero_grad_multi               sgd_zero_grad_block over the tensors of weight-decay
//                                       groups (those of the other groups own no block);
//   k_apply_entries_multi<kApply>       every entry takes its slot of acc (a gap's is dropped);
//                                       the winner applies fma(g, -lr, p) (wd == 0) or the
//                                       fix-up from its stash (wd != 0).
namespace dgc {

constexpr int kApplyMaxGroups = 8;

struct ApplyGroups {
    SgdHyper h[kApplyMaxGroups];
    int32_t count;
};

// groups.h[g] without a dynamically indexed copy of the kernel arguments
__device__ __forceinline__ SgdHyper apply_group(const ApplyGroups& groups, int32_t g) {
    SgdHyper h = groups.h[0];
#pragma unroll
    for (int j = 1; j < kApplyMaxGroups; ++j)
        if (g == j) h = groups.h[j];
    return h;
}

// The row holding flat index i: the last row with offset <= i, if i is inside it; else -1 (a
// padding gap, or a row whose group is out of range).
__device__ __forceinline__ int apply_row_of(const dgc_apply_row* __restrict__ rows, int32_t count, int64_t i,
                                            int32_t groups) {
    int lo = 0, hi = count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rows[mid].offset <= i) lo = mid;
        else hi = mid;
    }
    const int64_t j = i - rows[lo].offset;
    if (j < 0 || j >= rows[lo].numel || (uint32_t)rows[lo].group >= (uint32_t)groups) return -1;
    return lo;
}

template <int ID, int MODE>
__global__ void __launch_bounds__(kBlock)
k_apply_entries_multi(ApplySrc src, float* __restrict__ acc, const dgc_apply_row* __restrict__ rows, int32_t count,
                      float* __restrict__ stash, int64_t n, ApplyGroups groups) {
    const int r = (int)blockIdx.y;
    const char* base = src.payload + (int64_t)r * src.stride;
    const long long cnt = payload_count(base, src.capacity);
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < cnt; e += (long long)gridDim.x * kBlock) {
        const long long i = load_wire_idx<ID>(base + src.ioff, e);
        if (i < 0 || i >= n) continue;
        const int t = apply_row_of(rows, count, i, groups.count);
        const int64_t q = (int64_t)r * src.capacity + e;
        if (MODE == kApplyStash) {
            if (t < 0) continue;
            if (apply_group(groups, rows[t].group).wd != 0.f) stash[q] = rows[t].param[i - rows[t].offset];
            continue;
        }
        const uint32_t gb = __hip_atomic_exchange(reinterpret_cast<uint32_t*>(acc + i), 0u, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_AGENT);
        if (gb == 0u || t < 0) continue;   // +0.0 (as in k_apply_entries), or a gap's sum, dropped
        const float g = __uint_as_float(gb);
        const SgdHyper h = apply_group(groups, rows[t].group);
        float* p = rows[t].param + (i - rows[t].offset);
        if (h.wd == 0.f) {
            *p = __fmaf_rn(g, h.neg_lr, *p);
        } else {
            const bool mom = h.mom != 0.f;
            *p = sgd_fixup(stash[q], g, mom ? rows[t].momentum_buffer[i - rows[t].offset] : 0.f, mom, h);
        }
    }
}

__global__ void __launch_bounds__(kBlock)
k_sgd_zero_grad_multi(const dgc_apply_row* __restrict__ rows, int32_t count, ApplyGroups groups) {
    // the tensor of this block: the last row with block0 <= blockIdx.x (rows without blocks
    // share their block0 with the row after them, so they are never the last)
    const int64_t b = (int64_t)blockIdx.x;
    int lo = 0, hi = count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rows[mid].block0 <= b) lo = mid;
        else hi = mid;
    }
    const int64_t local = b - rows[lo].block0, n = rows[lo].numel;
    if (local < 0 || local * kSgdPerBlock >= n || (uint32_t)rows[lo].group >= (uint32_t)groups.count) return;
    const SgdHyper h = apply_group(groups, rows[lo].group);
    if (h.wd == 0.f) return;
    if (h.mom != 0.f)
        sgd_zero_grad_block<true>(rows[lo].param, rows[lo].momentum_buffer, n, rows[lo].first != 0, h, local);
    else
        sgd_zero_grad_block<false>(rows[lo].param, nullptr, n, false, h, local);
}

template <int ID>
static int apply_packed_multi(const ApplySrc& src, int32_t world, float* acc, int64_t n, const dgc_apply_row* rows,
                              int32_t count, int64_t dense_blocks, const ApplyGroups& groups, bool any_wd,
                              float* stash, hipStream_t s) {
    const dim3 grid((unsigned)grid_for(src.capacity, kBlock, kMaxGrid / 2), (unsigned)world), block(kBlock);
    const bool entries = src.capacity > 0;
    if (any_wd) {
        if (entries) {
            hipLaunchKernelGGL((k_apply_entries_multi<ID, kApplyStash>), grid, block, 0, s, src, acc, rows, count,
                               stash, n, groups);
            DGC_LAUNCHED();
        }
        if (dense_blocks > 0) {
            hipLaunchKernelGGL(k_sgd_zero_grad_multi, dim3((unsigned)dense_blocks), block, 0, s, rows, count, groups);
            DGC_LAUNCHED();
        }
    }
    if (entries) {
        hipLaunchKernelGGL((k_apply_entries_multi<ID, kApply>), grid, block, 0, s, src, acc, rows, count, stash, n,
                           groups);
        DGC_LAUNCHED();
    }
    return DGC_OK;
}

}  // namespace dgc

extern "C" size_t dgc_apply_packed_multi_workspace(int32_t world, int64_t capacity) {
    return dgc::apply_workspace(world, capacity);
}

extern "C" int dgc_apply_packed_multi(const void* payload, int32_t world, int64_t rank_stride, int64_t capacity,
                                      int32_t vdtype, int32_t idtype, float* acc, int64_t flat_numel,
                                      const dgc_apply_row* table, int32_t count, int64_t dense_blocks,
                                      const dgc_apply_hyper* hypers, int32_t groups, void* ws, size_t ws_bytes,
                                      void* stream) {
    using namespace dgc;
    static_assert(sizeof(dgc_apply_row) == 48, "dgc_apply_row is mirrored by dgc/_lib.py");
    if (!payload || !acc || !table || !hypers)
        DGC_FAIL(DGC_ERR_INVALID, "dgc_apply_packed_multi: null payload, acc, table or hypers");
    if (world < 1 || world > 64) DGC_FAIL(DGC_ERR_INVALID, "dgc_apply_packed_multi: world %d outside 1..64", world);
    DGC_TRY(check_wire("dgc_apply_packed_multi", vdtype, idtype));
    if (capacity < 0 || count < 1 || flat_numel < 1)
        DGC_FAIL(DGC_ERR_INVALID, "dgc_apply_packed_multi: capacity < 0, count < 1 or flat_numel < 1");
    if (groups < 1 || groups > kApplyMaxGroups)
        DGC_FAIL(DGC_ERR_INVALID, "dgc_apply_packed_multi: %d parameter groups outside 1..%d", groups, kApplyMaxGroups);
    if (dense_blocks < 0 || dense_blocks > 0x7FFFFFFFLL)
        DGC_FAIL(DGC_ERR_INVALID, "dgc_apply_packed_multi: dense_blocks outside [0, 2^31)");
    int64_t ioff = 0;
    const int64_t min_stride = payload_layout(capacity, vdtype, idtype, nullptr, &ioff);
    DGC_TRY(check_stride("dgc_apply_packed_multi", rank_stride, min_stride));
    ApplyGroups gs{};
    gs.count = groups;
    bool any_wd = false;
    for (int32_t g = 0; g < groups; ++g) {
        // lr >= 0 (a NaN fails too): the skip of a +0.0 slot needs -lr to carry the sign bit
        if (!(hypers[g].lr >= 0.f)) DGC_FAIL(DGC_ERR_INVALID, "dgc_apply_packed_multi: group %d: lr must be >= 0", g);
        gs.h[g] = SgdHyper{hypers[g].weight_decay, hypers[g].momentum, 1.f - hypers[g].dampening, -hypers[g].lr,
                           hypers[g].nesterov};
        any_wd = any_wd || hypers[g].weight_decay != 0.f;
    }
    const size_t need = apply_workspace(world, capacity);
    if (any_wd && (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 255)))
        DGC_FAIL(DGC_ERR_WORKSPACE, "dgc_apply_packed_multi: weight decay needs a workspace of %zu bytes, 256-B aligned",
                 need);
    const ApplySrc src{static_cast<const char*>(payload), rank_stride, ioff, capacity};
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* stash = static_cast<float*>(ws);
    return with_id(idtype, [&](auto ID) {
        return apply_packed_multi<ID()>(src, world, acc, flat_numel, table, count, dense_blocks, gs, any_wd, stash, s); });
}
