// Selection, K1 for 16-bit state (bf16 / fp16): k_compensate_list16, the flat bucket's
// one-tensor K1 over 16-bit momentum / velocity / gradient. Its own: how a tile is loaded,
// compensated (k_compensate16's arithmetic, half.hip: each of the reference's ops in fp32,
// rounded to the dtype) and stored, and the new velocity's exact fp32 image, which it
// writes. The strided sample, the sample window, the candidate lists and the segment's end
// are taken from that image by select_k1.hpp's shared steps (k1_segment_begin, k1_sample,
// k1_window_append, k1_segment_end), the ones k_compensate_list runs, so
// dgc_compress_finish serves the image unchanged.
//
// Layout: the fp32 kernel's. One wave per segment, element group (4 elements) index =
// 256*seg + 64*u + lane (u = 0..3): an 8-B load per lane and array, 512 B contiguous per
// instruction, and the image goes out as the fp32 kernel's 16-B store. The lane-to-element
// mapping, hence list_append, the sample arithmetic and the list order, are shared with
// the fp32 kernel. (16-B loads, 8 elements per lane, would halve the load count but need
// their own prefix over 8 predicate bits per lane; DESIGN.md §4 "K1-16".)
//
// Schedule: as select_k1.hpp documents — the state words (speculation thresholds, epoch)
// and the wave's twelve 8-B streaming loads go out through global-typed pointers before
// the first wait or store. That is 6 KB in flight per wave where the fp32 kernel has 12, so
// the launch keeps the register-limited occupancy (select.hip, compress_begin16).
//
// Bounds: the bucket pads momentum, velocity and image to a multiple of kSeg, so a live
// wave loads and stores whole groups of them. The gradient is exactly n elements: its full
// groups are 8-B loads, its partial last group is read element by element up to n (ld_tail16).
// Elements past n compute from zeros and are stored as +0; they are never sampled, listed
// or counted. The n & 3 elements of a partial group are compensated and sampled here (the
// fp32 path does both in separate launches) but, like there, not listed or windowed: their
// segment is marked spilled (d.tail).
//
// The 16-bit state is stored non-temporal whatever the size: a write-through (sc1) store
// narrower than 16 B is one fabric write each (MI355X_MICROARCH.md, stores), 2.7x the time
// per byte at 8 B. The image's 16-B store follows the fp32 kernel's rule (wt).
//
// No deferred masking: the 16-bit state is masked from the payload right after the
// selection (dgc_mask_packed16), which runs pure on the image.
//
// CLIP: the gradient clipped once it is unpacked, as the reference's clip leaves a 16-bit
// tensor (clip16, dgc_common.hpp: the product rounded to the dtype; the clamp against the bound rounded to
// the dtype). The tensor's coefficient is one more state word: a wave-uniform load issued
// with the others, ahead of the streaming loads and of every store (a null table is
// replaced by the tensor's own state, as K1 does). DGC_CLIP_NONE compiles to the unclipped
// kernel.
#pragma once
#include "select_k1.hpp"

namespace dgc {
// x holds values of the dtype (round16's results): the narrowing is exact
template <int DT>
__device__ __forceinline__ uint2 pack4(const float (&x)[4]) {
    return make_uint2((uint32_t)f32_to_h16<DT>(x[0]) | ((uint32_t)f32_to_h16<DT>(x[1]) << 16),
                      (uint32_t)f32_to_h16<DT>(x[2]) | ((uint32_t)f32_to_h16<DT>(x[3]) << 16));
}

// The last group of a gradient that ends inside it (exactly n elements, n & 3 of them in
// this group, which starts at element 4 * (n / 4)): elements past n read as +0. 2-B loads:
// an 8-B load would run past the gradient's end.
__device__ __forceinline__ uint2 ld_tail16(DGC_GLB const uint16_t* g, int64_t n) {
    DGC_GLB const uint16_t* p = g + (n & ~(int64_t)3);
    const int r = (int)(n & 3);
    return make_uint2((uint32_t)p[0] | (r > 1 ? (uint32_t)p[1] << 16 : 0u), r > 2 ? (uint32_t)p[2] : 0u);
}

// DGCSGDMemory.compensate on one 16-bit element, as k_compensate16 (half.hip) does it
template <int DT, bool NEST>
__device__ __forceinline__ float comp16(float g, float& m, float& v, float mom) {
    if (NEST) {   // mmt.add_(grad).mul_(m); vec.add_(mmt).add_(grad)
        m = round16<DT>(__fadd_rn(m, g));
        m = round16<DT>(__fmul_rn(m, mom));
        v = round16<DT>(__fadd_rn(v, m));
        v = round16<DT>(__fadd_rn(v, g));
    } else {      // mmt.mul_(m).add_(grad); vec.add_(mmt)
        m = round16<DT>(__fmul_rn(m, mom));
        m = round16<DT>(__fadd_rn(m, g));
        v = round16<DT>(__fadd_rn(v, m));
    }
    return v;
}

template <int DT, bool NEST, int CLIP>
__global__ void __launch_bounds__(kBlock)
k_compensate_list16(const uint16_t* __restrict__ g16, uint16_t* __restrict__ mmt16, uint16_t* __restrict__ vec16,
                    float* __restrict__ img, float mom, SelWS w, int64_t start, int wt, OneTable ot, ClipArg ca) {
    const TDesc d = ot.d;   // by value: stores below cannot alias it
    const int lane = threadIdx.x & 63, wave = wave_id();
    const int64_t ls = (int64_t)blockIdx.x * kSegPerBlock4 + wave;   // local segment
    // a wave past the last segment loads nothing and lists nothing (no early exit: a
    // branch here would split the state reads from the streaming loads)
    const bool live = ls < d.nseg;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    const bool sample = d.samp_off >= 0;

    // ---- the state words
    DGC_GLB SelState* st = glb(w.st);
    DGC_GLB const float* spec = w.spec ? glb(w.spec) : &st->t0;   // (null: any readable words)
    const float spec0 = spec[0], spec2 = spec[2];
    const int32_t epoch = st->epoch;
    float cf_tab = 0.f;
    if (CLIP != DGC_CLIP_NONE) cf_tab = *(ca.tab ? glb(ca.tab) : (DGC_GLB const float*)&st->t0);

    // ---- the streaming loads: momentum and velocity (padded: whole groups), then the
    // gradient's full groups
    const int64_t n = d.n;
    const int64_t seg4 = ls * (kSeg / 4);
    const int gleft = (int)min((n >> 2) - seg4, (int64_t)(kSeg / 4));   // full groups of the gradient here
    DGC_GLB u2v* mmt = glb(reinterpret_cast<u2v*>(mmt16) + seg4);
    DGC_GLB u2v* vec = glb(reinterpret_cast<u2v*>(vec16) + seg4);
    DGC_GLB const u2v* g = glb(reinterpret_cast<const u2v*>(g16) + seg4);
    DGC_GLB float4* im = glb(reinterpret_cast<float4*>(img) + seg4);
    // (read below only where loaded: merging a load with a constant here would make the
    // compiler wait for it on the spot)
    uint2 gv[kSegTiles], mv[kSegTiles], vv[kSegTiles];
#pragma unroll
    for (int u = 0; u < kSegTiles; ++u) {
        if (live) {
            mv[u] = ld_nt(mmt + u * 64 + lane);
            vv[u] = ld_nt(vec + u * 64 + lane);
        }
    }
#pragma unroll
    for (int u = 0; u < kSegTiles; ++u)
        if (u * 64 + lane < gleft) gv[u] = ld_nt(g + u * 64 + lane);
    // the one wave that owns the gradient's partial last group reads it into registers
    // of its own (wave-uniform branch, one lane loads)
    const bool tailw = (n & 3) && gleft >= 0 && gleft < kSeg / 4;
    uint2 gt = make_uint2(0u, 0u);
    if (tailw && lane == (gleft & 63)) gt = ld_tail16(glb(g16), n);

    // ---- everything loaded is in flight: the stores of the call's tables
    if (first) {
        w.td[0] = ot.d;
        for (int which = 0; which < BT_COUNT; ++which) {
            w.bt[which][0] = ot.bt[which][0];
            w.bt[which][1] = ot.bt[which][1];
        }
        w.small[0] = 0;
    }
    if (!sample) start = 0;
    const int64_t scount = !sample ? 0 : ceil_div(d.n - start, d.stride);
    const K1Seg k = k1_segment_begin(w, d, 0, st, first, true, spec0, spec2, epoch, ls, start, scount);
    uint32_t c = 0, mk = 0;
    const int64_t seg = d.seg0 + ls;
    const float cf = clip_bound16<DT, CLIP>(ca, cf_tab);
#pragma unroll
    for (int u = 0; u < kSegTiles; ++u) {
        const int64_t e = 4 * (seg4 + u * 64 + lane);
        // elements of the group inside the tensor
        const uint32_t valid =
            !live ? 0u : (e + 3 < n ? 0xFu : (e + 2 < n ? 7u : (e + 1 < n ? 3u : (e < n ? 1u : 0u))));
        // a partial group is compensated and sampled, but not listed or windowed: its
        // segment is marked spilled (d.tail)
        const uint32_t lvalid = valid == 0xFu ? 0xFu : 0u;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        bool hit = false;   // this lane's sample (at most one per group: stride >= 4) joins the window
        float hv = 0.f;
        if (valid) {
            float gx[4], mx[4];
            const int gi = u * 64 + lane;
            unpack4<DT>(gi < gleft ? gv[u] : (tailw && gi == gleft ? gt : make_uint2(0u, 0u)), gx);
            unpack4<DT>(mv[u], mx);
            unpack4<DT>(vv[u], x);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                comp16<DT, NEST>(clip16<DT, CLIP>(gx[j], cf), mx[j], x[j], mom);
                if (!((valid >> j) & 1u)) mx[j] = x[j] = 0.f;   // padding stays +0
            }
            st_nt(mmt + u * 64 + lane, pack4<DT>(mx));
            st_nt(vec + u * 64 + lane, pack4<DT>(x));
            st_stream(im + u * 64 + lane, make_float4(x[0], x[1], x[2], x[3]), wt);
            if (sample) hit = k1_sample(k, d, x, valid, u * 64 + lane, k.windowed && lvalid, hv);
        }
        k1_window_append(k, d.win_cap, hit, hv, lane);
        list_append(ge_mask(x, lvalid, k.tl), x, u * 256, c, w.lst_off, w.lst_val, seg);
        mk = max(mk, tile_max_key(x, lvalid));
    }
    k1_segment_end(c, mk, lane == 0 && live, d.tail && ls == d.nseg - 1, w.seg_lcnt + seg, w.st[0].spill[epoch & 1]);
}
}  // namespace dgc
