// The packed payload [count | order | values | indices] and the wire dtypes, in one place: its layout,
// the argument checks every entry point that takes one repeats, and the device-side reads of
// its header, its indices and its values.
//
//   bytes 0..7    int64 count (a gathered header is clamped to [0, capacity] by its readers)
//   bytes 8..15   int64 order word (DGC_ORDER_ASCENDING; a split part: the bound of the later parts)
//   voff = 16     `capacity` values of the wire value dtype
//   ioff          `capacity` indices, 16-B aligned; the whole payload is a multiple of 256 B
#pragma once

#include "dgc_common.hpp"

namespace dgc {

// ------------------------------------------------------------------ host: layout and checks
constexpr int vbytes(int vd) { return vd == DGC_F32 ? 4 : 2; }   // F16, BF16: 2
constexpr int ibytes(int id) { return id == DGC_I32 ? 4 : 8; }
inline bool is16(int dt) { return dt == DGC_BF16 || dt == DGC_F16; }
inline bool index_ok(int id) { return id == DGC_I64 || id == DGC_I32; }
// any dtype of the library's floats (a parameter dtype, a threshold dtype, a cast's destination): not a wire check,
// so a new wire dtype does not widen it by accident
inline bool float_dtype_ok(int dt) { return dt == DGC_F32 || dt == DGC_F16 || dt == DGC_BF16; }
// a wire value dtype: fp32 or fp16, and bf16 where the receiver is a 16-bit parameter
inline bool wire_ok(int vd, bool bf16) { return vd == DGC_F32 || vd == DGC_F16 || (bf16 && vd == DGC_BF16); }

// Offsets of the values and the indices; returns the payload's bytes (decompress.hip).
int64_t payload_layout(int64_t capacity, int vd, int id, int64_t* voff, int64_t* ioff);

// The refusals that are worded the same at every entry point; `who` is the entry point's name.
// (An entry point that words one differently keeps its own line.)
inline int check_wire(const char* who, int vd, int id, bool bf16 = false) {
    if (!wire_ok(vd, bf16) || !index_ok(id)) DGC_FAIL(DGC_ERR_DTYPE, "%s: unsupported value/index dtype (%d, %d)", who, vd, id);
    return DGC_OK;
}
inline int check_stride(const char* who, int64_t rank_stride, int64_t layout) {
    if (rank_stride < layout)
        DGC_FAIL(DGC_ERR_INVALID, "%s: rank_stride %lld < layout %lld", who, (long long)rank_stride, (long long)layout);
    return DGC_OK;
}
// what: "dtype", or "grad dtype" on the receive side
inline int check_h16(const char* who, int dt, const char* what = "dtype") {
    if (!is16(dt)) DGC_FAIL(DGC_ERR_DTYPE, "%s: %s must be DGC_BF16 or DGC_F16", who, what);
    return DGC_OK;
}
// The clip kinds of a fused clip: SCALE needs the coefficient table, CLAMP a table or a value.
inline int check_clip(const char* who, int kind, const float* clip) {
    if (!clip_kind_ok(kind)) DGC_FAIL(DGC_ERR_INVALID, "%s: clip kind %d", who, (int)kind);
    if (kind == DGC_CLIP_SCALE && !clip) DGC_FAIL(DGC_ERR_INVALID, "%s: DGC_CLIP_SCALE needs the coefficient table", who);
    return DGC_OK;
}

// ------------------------------------------------------------------ device: reads
// Entry e of an index / value array in global memory (typed: global_ loads).
template <int ID>
__device__ __forceinline__ long long load_idx(const void* p, long long e) {
    if (ID == DGC_I32) return ((const DGC_GLB int32_t*)p)[e];
    return ((const DGC_GLB int64_t*)p)[e];
}
template <int VD>
__device__ __forceinline__ float load_val(const void* p, long long e) {
    if (VD == DGC_F16) return (float)((const DGC_GLB _Float16*)p)[e];   // exact widening
    if (VD == DGC_BF16) return bf16_to_f32(((const DGC_GLB uint16_t*)p)[e]);   // (a 16-bit receiver's wire only)
    return ((const DGC_GLB float*)p)[e];
}
// The same reads through generic pointers (half.hip's rank-by-rank port, sgd.hip's sparse step):
// what those kernels were built and measured with; moving them to the typed loads is its own change.
template <int VD>
__device__ __forceinline__ float load_wire(const void* values, int64_t e) {
    if (VD == DGC_F32) return static_cast<const float*>(values)[e];
    if (VD == DGC_F16) return f16_to_f32(static_cast<const uint16_t*>(values)[e]);
    return bf16_to_f32(static_cast<const uint16_t*>(values)[e]);
}
template <int ID>
__device__ __forceinline__ long long load_wire_idx(const void* indices, long long e) {
    if (ID == DGC_I32) return static_cast<const int32_t*>(indices)[e];
    return static_cast<const int64_t*>(indices)[e];
}

// The header's count as it stands, and clamped to the capacity its buffer was laid out for.
__device__ __forceinline__ long long payload_count_raw(const char* payload) {
    return *reinterpret_cast<const long long*>(payload);
}
__device__ __forceinline__ long long payload_count(const char* payload, long long capacity) {
    const long long c = payload_count_raw(payload);
    return c < 0 ? 0 : (c > capacity ? capacity : c);
}

// Chunk tables (a launch over <= 64 tensors that rides in the kernel arguments, tensor t's
// workgroups from c.bstart[t]): the tensor of workgroup b, bstart[t] <= b < bstart[t + 1].
// Takes the table itself, not a pointer into it: the reads stay kernel-argument loads.
template <typename C>
__device__ __forceinline__ int chunk_of(const C& c, int b) {
    int lo = 0, hi = c.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (c.bstart[mid] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace dgc
