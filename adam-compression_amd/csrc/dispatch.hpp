// Host only: the one place where a run-time dtype, index type or flag becomes a template
// argument. Every with_*(x, f) calls the generic lambda f with a tag (an
// std::integral_constant) whose value is a constant expression inside f:
//
//   with_h16(dtype, [&](auto DT) { with_clip(kind, [&](auto CLIP) {
//       hipLaunchKernelGGL((k_compensate16_mt<DT(), NEST(), CLIP()>), ...); }); });
//
// and returns what f returns. The domains differ on purpose: each takes exactly the values its
// callers' kernels are instantiated for, so a new call site cannot pull in a superset.
// Arguments are validated BEFORE dispatch (payload.hpp's checks): a dispatcher never discovers
// a bad value, its last arm is simply the remaining member of the domain.
#pragma once

#include <cstdint>
#include <type_traits>

#include "dgc_hip.h"

namespace dgc {

template <int V>
using Tag = std::integral_constant<int, V>;

// An index dtype: the DGC_I32 / DGC_I64 constant, and the C type for kernels templated on it.
template <int ID>
struct IdxTag : Tag<ID> {
    using type = std::conditional_t<ID == DGC_I32, int32_t, int64_t>;
};
template <class T>
using idx_t = typename T::type;

template <class F>
decltype(auto) with_bool(bool b, F&& f) {
    if (b) return f(std::true_type{});
    return f(std::false_type{});
}

// a kernel's mode: 0 .. N - 1
template <int N, class F>
decltype(auto) with_mode(int m, F&& f) {
    if constexpr (N > 1) {
        if (m == N - 1) return f(Tag<N - 1>{});
        return with_mode<N - 1>(m, f);
    } else {
        return f(Tag<0>{});
    }
}

// index dtype: DGC_I32 | DGC_I64
template <class F>
decltype(auto) with_id(int id, F&& f) {
    if (id == DGC_I32) return f(IdxTag<DGC_I32>{});
    return f(IdxTag<DGC_I64>{});
}

// wire value dtype of the fp32 receive side: DGC_F32 | DGC_F16
template <class F>
decltype(auto) with_vd(int vd, F&& f) {
    if (vd == DGC_F16) return f(Tag<DGC_F16>{});
    return f(Tag<DGC_F32>{});
}

// wire value dtype of the 16-bit receive side: DGC_F32 | DGC_F16 | DGC_BF16
template <class F>
decltype(auto) with_wire16(int vd, F&& f) {
    if (vd == DGC_F32) return f(Tag<DGC_F32>{});
    if (vd == DGC_F16) return f(Tag<DGC_F16>{});
    return f(Tag<DGC_BF16>{});
}

// a 16-bit parameter dtype: DGC_BF16 | DGC_F16
template <class F>
decltype(auto) with_h16(int dt, F&& f) {
    if (dt == DGC_BF16) return f(Tag<DGC_BF16>{});
    return f(Tag<DGC_F16>{});
}

// clip kind of a fused clip: DGC_CLIP_NONE | DGC_CLIP_SCALE | DGC_CLIP_CLAMP
template <class F>
decltype(auto) with_clip(int kind, F&& f) {
    if (kind == DGC_CLIP_SCALE) return f(Tag<DGC_CLIP_SCALE>{});
    if (kind == DGC_CLIP_CLAMP) return f(Tag<DGC_CLIP_CLAMP>{});
    return f(Tag<DGC_CLIP_NONE>{});
}

// clip kind of a clip on its own (dgc_clip_apply: there is no NONE kernel): SCALE | CLAMP
template <class F>
decltype(auto) with_clip_on(int kind, F&& f) {
    if (kind == DGC_CLIP_SCALE) return f(Tag<DGC_CLIP_SCALE>{});
    return f(Tag<DGC_CLIP_CLAMP>{});
}

}  // namespace dgc
