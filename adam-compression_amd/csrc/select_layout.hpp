// Selection, host layout: what the host derives from the tensor list — TensorIn, Layout,
// bt_blocks / build_layout (the device table image and the block tables) and
// carve_select (the workspace carve) — and the two kernels that put a call's tables and
// sample starts on the device (OneTable / k_put_one, StartChunk / k_put_starts; K1 takes
// both structs in its arguments). Recomputed on every call (O(T)). Relies on
// select_types.hpp.
#pragma once
#include <algorithm>
#include <vector>
#include "select_types.hpp"

namespace dgc {
struct TensorIn {
    int64_t n, off, k, S, ks, stride, upper_count, lower_count;
    bool samples;   // reserve a sample buffer (compress); false for a pure selection
};

struct Layout {
    int32_t T = 0;
    int64_t nseg = 0, ngrp = 0, nsamp = 0, ncand = 0, ngpos = 0;
    int64_t max_cand = 0;       // the largest K5 candidate capacity of a tensor
    int64_t max_k = 0;          // the largest num_selects
    int32_t nsmall = 0;
    int32_t nwins = 0;          // tensors with a K1 sample window (their ids follow the small ones)
    int32_t nplain = 0;         // multi-block threshold tasks without a window (k_rs_reset_samples)
    bool adapt_any = false;     // some tensor has N > S (the adaptation loop can run)
    bool tail_any = false;      // some tensor is compensated partly outside K1 (unpadded tail)
    int64_t grid[BT_COUNT] = {};
};

// Capped grids serve the launches that are most likely gated no-ops (the list count
// usually serves), so a small grid keeps their cost down — for a flat bucket, whose
// lists serve in the steady state. A model set's passes run most steps (its synthetic
// thresholds jump), and there a 2048-block cap left the big tensors' passes
// short of HBM rate: 8192 blocks took VGG-16-BN 0.896 -> 0.811 ms, ResNet-50 0.367 ->
// 0.361 ms, 16384 VGG-16-BN 0.816 -> 0.805 ms, ResNet-50 unchanged (same box).
// K5s: the fewest workgroups of a cooperative set (beyond kSetCoopMin candidates) — the
// grid holds max(this, ceil(capacity / kSetCoopMin)) per tensor. 16 per tensor made a
// ResNet-50 step dispatch ~430 workgroups of 1024 threads, and its biggest sets started
// 12-14 us into the launch (tools/k5s_prof.py): kSetGDefault.

static inline int64_t bt_blocks(int which, const TDesc& d, int64_t total_seg, int64_t cap_blocks) {
    const int64_t cap = std::max<int64_t>(1, ceil_div(cap_blocks * d.nseg, std::max<int64_t>(1, total_seg)));
    switch (which) {
        case BT_K1: return ceil_div(d.nseg, (int64_t)kSegPerBlock4);
        case BT_FULL: return ceil_div(d.nseg, (int64_t)kSegPerBlock16);
        case BT_CAP16: return std::min(ceil_div(d.nseg, (int64_t)kSegPerBlock16), cap);
        case BT_CAP4: return std::min(ceil_div(d.nseg, (int64_t)kSegPerBlock4), cap);
        case BT_FULL8: return ceil_div(d.nseg, (int64_t)(2 * kSegPerBlock4));
        case BT_CAP8: return std::min(ceil_div(d.nseg, (int64_t)(2 * kSegPerBlock4)), cap);
        case BT_SEG: return ceil_div(d.nseg, (int64_t)kBlock);
        case BT_CNT: return ceil_div(d.nseg, (int64_t)kBlock * kCountSegs);
        case BT_GRP: return ceil_div(d.nseg, (int64_t)(kGroupSegs / kEmitSplit));
        case BT_QUEUE: return ceil_div(d.k, (int64_t)kQueuePerBlock);
        case BT_SET:   // K5s: a resample set holds count(t_cur) <= cand_cap > k candidates
            if (d.k < 1 || d.cand_cap <= d.k) return 0;
            if (d.cand_cap <= kSetCoopMin) return 1;
            return std::min<int64_t>(kSetGBig, std::max<int64_t>(kSetGDefault, ceil_div(d.cand_cap, kSetCoopMin)));
        case BT_SAMP: {
            const int64_t cnt = d.samp_off < 0 ? d.n : d.S + 1;
            if (cnt <= kSmallN) return 0;   // one-workgroup threshold (k_rs_small_multi)
            return std::min<int64_t>(512, ceil_div(cnt, (int64_t)kBlock * 16));
        }
    }
    return 0;
}

static void build_layout(const TensorIn* in, int32_t T, bool padded, Layout& L, std::vector<TDesc>& td,
                         std::vector<int32_t> (&bt)[BT_COUNT], std::vector<int32_t>& small) {
    L = Layout{};
    L.T = T;
    td.assign(T, TDesc{});
    small.clear();
    int64_t seg_end = 0, grp = 0, samp = 0, cand = 0, gpos = 0;
    for (int32_t t = 0; t < T; ++t) {
        TDesc& d = td[t];
        d.n = in[t].n;
        d.off = in[t].off;
        d.seg0 = d.off / kSeg;
        d.nseg = ceil_div(d.n, (int64_t)kSeg);
        d.grp0 = grp;
        d.ngrp = ceil_div(d.nseg, (int64_t)kGroupSegs);
        grp += d.ngrp;
        d.k = in[t].k;
        d.S = in[t].S;
        d.ks = in[t].ks;
        d.stride = in[t].stride;
        d.upper_count = in[t].upper_count;
        d.lower_count = in[t].lower_count;
        const bool sampled = d.n != d.S;
        L.adapt_any |= sampled;
        d.samp_off = (sampled && in[t].samples) ? samp : -1;
        if (d.samp_off >= 0) samp += (int64_t)align_up((size_t)(d.S + 1), 64);
        // a window list for the multi-block thresholds; its size cannot depend on ks
        // (dgc_compress_begin lays the workspace out without it)
        d.win_cap = (d.samp_off >= 0 && d.S + 1 > kSmallN) ? std::min<int64_t>(d.S + 1, (d.S + 1) / 16 + 4096) : 0;
        d.win_off = samp;
        samp += (int64_t)align_up((size_t)d.win_cap, 64);
        d.whist_off = samp;
        if (d.win_cap > 0) samp += kWinBins;
        d.cand_off = cand;
        d.cand_cap = nth_cand_cap(d.n, d.k);
        cand += d.cand_cap;
        L.max_cand = std::max(L.max_cand, d.cand_cap);
        L.max_k = std::max(L.max_k, d.k);
        d.gpos_off = gpos;
        gpos += 2 * (d.cand_cap / 2 + 1);
        d.idx_base = T > 1 ? d.off : 0;
        d.nv4 = padded ? ceil_div(d.n, (int64_t)4) : d.n / 4;
        d.tail = (!padded && (d.n & 3)) ? 1 : 0;
        L.tail_any |= d.tail != 0;
        d.inv_stride = 1.0 / (double)(d.stride > 0 ? d.stride : 1);
        d.inv_stride_f = 1.0f / (float)(d.stride > 0 ? d.stride : 1);
        seg_end = std::max(seg_end, d.seg0 + d.nseg);
        const int64_t scnt = sampled ? d.S + 1 : d.n;
        if (scnt <= kSmallN) small.push_back(t);
        else if (!(d.win_cap > 0 && !d.tail)) ++L.nplain;
    }
    L.nseg = seg_end;
    L.ngrp = grp;
    L.nsamp = samp;
    L.ncand = cand;
    L.ngpos = gpos;
    L.nsmall = (int32_t)small.size();
    // the windowed tensors after the small ones: k_rs_small_multi tries their windows
    for (int32_t t = 0; t < T; ++t)
        if (td[t].win_cap > 0 && !td[t].tail) small.push_back(t);
    L.nwins = (int32_t)small.size() - L.nsmall;
    for (int which = 0; which < BT_COUNT; ++which) {
        bt[which].assign(T + 1, 0);
        int64_t acc = 0;
        for (int32_t t = 0; t < T; ++t) {
            bt[which][t] = (int32_t)acc;
            acc += bt_blocks(which, td[t], L.nseg, T > 1 ? kCapBlocksBatch : kCapBlocks);
        }
        bt[which][T] = (int32_t)acc;
        L.grid[which] = acc;
    }
}

static SelWS carve_select(void* base, const Layout& L, size_t* bytes = nullptr) {
    SelWS w{};
    w.T = L.T;
    w.nseg = L.nseg;
    w.ngrp = L.ngrp;
    Carver c(base);
    w.td = c.take<TDesc>(L.T);
    w.st = c.take<SelState>(L.T);
    w.rs = c.take<RSState>(L.T);
    w.thr = c.take<float>(L.T);
    w.spec = c.take<float>(kSpecWords * L.T);
    w.starts = c.take<int64_t>(L.T);
    w.gptr = c.take<const float*>(L.T);
    w.scnt = c.take<int64_t>(L.T);
    for (int which = 0; which < BT_COUNT; ++which) w.bt[which] = c.take<int32_t>(L.T + 1);
    w.small = c.take<int32_t>(L.T);
    w.samples = c.take<float>(L.nsamp);
    w.grp_cnt = c.take<unsigned long long>(L.ngrp);
    w.grp_off = c.take<long long>(L.ngrp);
    w.grp_lb = c.take<unsigned long long>(L.ngrp);
    w.seg_lcnt = c.take<uint32_t>(L.nseg);
    w.seg_cnt = c.take<uint32_t>(L.nseg);
    w.seg_off = c.take<uint32_t>(L.nseg);
    w.lst_off = c.take<uint16_t>(ceil_div(L.nseg, (int64_t)kLstTile) * kLstTile * kCap);
    w.lst_val = c.take<float>(ceil_div(L.nseg, (int64_t)kLstTile) * kLstTile * kCap);
    w.queue = c.take<uint64_t>(L.ncand);
    w.cand_idx = c.take<int64_t>(L.ncand);
    w.cand_val = c.take<float>(L.ncand);
    w.cand_key = c.take<uint32_t>(L.ncand);
    w.gpos = c.take<uint32_t>(L.ngpos);
    w.nthg = c.take<NthG>(L.T);
    w.setg = c.take<SetG>(L.T);
    w.fin_ticket = c.take<uint32_t>(16);
    w.chain = c.take<uint32_t>(kChainWords);
    if (bytes) *bytes = c.bytes();
    return w;
}

// The tables of a one-tensor call, written by one tiny kernel (no host copy).
struct OneTable {
    TDesc d;
    int32_t bt[BT_COUNT][2];
    int64_t start;
};

__global__ void k_put_one(SelWS w, OneTable o) {
    if (threadIdx.x != 0) return;
    w.td[0] = o.d;
    for (int which = 0; which < BT_COUNT; ++which) {
        w.bt[which][0] = o.bt[which][0];
        w.bt[which][1] = o.bt[which][1];
    }
    w.small[0] = 0;
    w.starts[0] = o.start;
    const TDesc& d = o.d;
    w.scnt[0] = d.samp_off < 0 ? d.n : ceil_div(d.n - o.start, d.stride);
}

// Per-call sample starts of a batch (random.randint per tensor, drawn on the host),
// 64 per launch in the kernel arguments; also the sample counts. ptrs: K1 reads tensor
// t's gradient from grad[t] (a pointer table: the parameters' own p.grad tensors, no
// copy into the flat buffer) instead of the flat buffer at its offset.
struct StartChunk {
    int32_t first, count;
    int32_t ptrs, pad;
    int64_t start[64];
    const float* grad[64];
};

__global__ void k_put_starts(SelWS w, StartChunk c) {
    const int i = threadIdx.x;
    if (i >= c.count) return;
    const int t = c.first + i;
    const TDesc d = w.td[t];   // by value: stores below cannot alias it
    w.starts[t] = c.start[i];
    w.scnt[t] = d.samp_off < 0 ? d.n : ceil_div(d.n - c.start[i], d.stride);
    if (c.ptrs) w.gptr[t] = c.grad[i];
}
}  // namespace dgc
