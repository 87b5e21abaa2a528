// K1, channel-tiled form -- token rows wider than one workgroup (C / pack width > 1024 lanes: fp32 C > 4096, 16-bit C > 8192).
//
// The one-workgroup kernels (quadtree_spatial.inc) map one lane to one channel pack and keep a root cell's whole pyramid in VGPRs,
// so a row must fit 1024 lanes.  Here a row is cut into `nchunk` chunks of blockDim.x lanes and the stage runs in three launches:
//   pass A  k_wide_stats:  one workgroup per (frame, root cell, chunk).  Loads the chunk's leaves once, pools the pyramid in
//           registers with the general body's code (block_geometry / load_and_pool_block / block_stats / AliasPool, the same
//           slot order as k_spatial) and writes the chunk's NSTAT partial statistics (norms, parent . child dots, alias norms;
//           per-head: the per-head cosines summed over the chunk's heads) to a table at the start of S;
//   pass B  k_wide_decide: one workgroup per (frame, root cell).  Sums the chunk partials in fixed chunk order (no float atomics:
//           the same bits run to run) and runs decide_and_emit -- the one-workgroup kernels' own decision and metadata code --
//           which writes meta, inrm, rc_list, lab_row, gcnt, cgeo, frame_cnt and the counters;
//   pass C  k_wide_emit:   one workgroup per (frame, root cell, chunk).  Walks the root cell's node list and writes the chunk's
//           channels of every emitted node into S, pooled again from the leaves with pool4 in the pyramid's order (the feature
//           bits are those of the one-workgroup kernels).  1x1 nodes of a dense input stay in x, as there.
// The statistics table needs T * R * nchunk * NSTAT floats, far less than S (the host checks), and S is not written before pass C:
// the wide form needs no workspace of its own, so sttm_quadtree_workspace_bytes is the same for every shape.
// Pass C re-reads only the leaves under emitted nodes of more than one leaf (instead of staging the pooled non-leaf rows of
// pass A: DESIGN.md, "Rows wider than one workgroup").
// Heads of the per-head cosine are chunk-local: a chunk is a multiple of 64 lanes and a head is a power of two <= 64 lanes.
// Trees of at most 4 levels (every preset); deeper trees with wide rows are refused by the host.
#pragma once
#include "quadtree_spatial.inc"

namespace sttm {

// (4-level trees: at most 512 lanes per chunk -- the 4 block tops are live beside a whole block, and at 128 VGPRs the 16-byte
// instantiations spilled)
template <typename T, int VEC, int BL, int UL, bool PERHEAD>
__global__ void __launch_bounds__(UL == 0 ? 1024 : 512) k_wide_stats(const SpatialArgs a0, const BatchPtrs bp, int nchunk) {
    SpatialArgs a = a0;
    rebase(a, bp, blockIdx.y);
    constexpr int D = BL + UL;
    static_assert(UL <= 1, "the channel-tiled form takes trees of at most 4 levels");
    using TC = TreeConst<D>;
    constexpr int NSTAT = TC::NSTAT;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* part = reinterpret_cast<float*>(smem_raw);             // [nwave][NSTAT]
    const int nwave = blockDim.x / kWave;
    const LevelDims& g = a.dims;
    const int R = g.h[0] * g.w[0];
    const int item = blockIdx.x / nchunk, chunk = blockIdx.x - item * nchunk;
    const int t = item / R, rcell = item - t * R;
    const int I = rcell / g.w[0], J = rcell % g.w[0];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    SpatialCtx cx;
    spatial_ctx_init<T>(cx, a, t, chunk * (int)blockDim.x + tid, VEC);

    BlockGeo bg;
    BlockRegs<T, VEC> regs;
    Pack<T, VEC> alias[D];
    if constexpr (UL == 0) {
        block_geometry<BL>(g, 0, I, J, true, bg);
        load_block<T, VEC, BL>(cx, t, I, J, true, bg, regs);
    }
    for (int s = tid; s < nwave * NSTAT; s += blockDim.x) part[s] = 0.f;
    bool need_alias[D];
#pragma unroll
    for (int m = 0; m < D; ++m) {
        need_alias[m] = m >= 1 && (((g.h[m] & 1) && I == 0) || ((g.w[m] & 1) && J == 0));
        alias[m].zero();
    }
    if constexpr (D >= 2) if (need_alias[D - 1]) alias[D - 1] = AliasPool<T, VEC, 0>::run(cx, g, t, D - 1, 0, 0);
    if constexpr (D >= 3) if (need_alias[D - 2]) alias[D - 2] = AliasPool<T, VEC, 1>::run(cx, g, t, D - 2, 0, 0);
    if constexpr (D >= 4) if (need_alias[D - 3]) alias[D - 3] = AliasPool<T, VEC, 2>::run(cx, g, t, D - 3, 0, 0);
    lds_barrier();     // LDS cleared (the loads stay in flight)

    float* mypart = part + wave * NSTAT;
#pragma unroll
    for (int m = 1; m < D; ++m) {
        if (need_alias[m]) {
            const float tot = wave_sum(dot_pack(alias[m], alias[m]));
            if (lane == 0) mypart[TC::alias_id(m)] = tot;
        }
    }
    if constexpr (UL == 0) {
        pool_block<T, VEC, BL>(cx, true, bg, regs);
        block_stats<T, VEC, BL, D, PERHEAD>(regs, bg, true, 0, 0, alias, mypart, lane, a.head_lanes);
    } else {
        const CellGeo c0 = cell_children(g, 0, I, J);
        bool v0[4];
        Pack<T, VEC> upper[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v0[k] = (k >> 1) < c0.rc && (k & 1) < c0.cc;
            upper[k].zero();
            if (v0[k]) {
                block_geometry<BL>(g, 1, c0.rs + (k >> 1), c0.cs + (k & 1), true, bg);
                load_and_pool_block<T, VEC, BL>(cx, t, c0.rs + (k >> 1), c0.cs + (k & 1), true, bg, regs);
                block_stats<T, VEC, BL, D, PERHEAD>(regs, bg, true, 1 + k, 1, alias, mypart, lane, a.head_lanes);
                upper[k] = regs.top;
            }
        }
        const Pack<T, VEC> root = pool4<T, VEC>(upper, v0, cx.sum_mode);
        if constexpr (PERHEAD) {
            float s[4];
            head_parent_ratios<T, VEC>(root, upper, v0, alias[1], a.head_lanes, lane, s);
            const float tot = wave_reduce_many<4>(s, lane);
            bool ok;
            const int idx = wave_reduce_slot<4>(lane, ok);
            if (ok) mypart[TC::dot_id(0, idx)] = tot;
        } else {
            float s[5];
            s[0] = dot_pack(root, root);
#pragma unroll
            for (int k = 0; k < 4; ++k) s[1 + k] = v0[k] ? dot_pack(root, upper[k]) : dot_pack(root, alias[1]);
            const float tot = wave_reduce_many<5>(s, lane);
            bool ok;
            const int idx = wave_reduce_slot<5>(lane, ok);
            if (ok) mypart[idx == 0 ? 0 : TC::dot_id(0, idx - 1)] = tot;
        }
    }
    lds_barrier();
    // the chunk's statistics: its waves summed in a fixed order
    float* out = reinterpret_cast<float*>(a.S) + (int64_t)blockIdx.x * NSTAT;
    for (int s = tid; s < NSTAT; s += blockDim.x) {
        float acc = 0.f;
        for (int w = 0; w < nwave; ++w) acc += part[w * NSTAT + s];
        out[s] = acc;
    }
}

// pass B: the chunks of a (frame, root cell) are the "waves" of decide_and_emit's fixed-order sum
template <int D, bool PERHEAD>
__global__ void __launch_bounds__(256) k_wide_decide(const SpatialArgs a0, const BatchPtrs bp, int nchunk) {
    SpatialArgs a = a0;
    rebase(a, bp, blockIdx.y);
    using TC = TreeConst<D>;
    __shared__ double inrm_l[TC::NNODE];
    __shared__ float stat[TC::NSTAT];
    __shared__ int stop[TC::NPAR > 0 ? TC::NPAR : 1];
    __shared__ int orow[TC::NNODE];
    __shared__ int lcount[2];
    const LevelDims& g = a.dims;
    const int R = g.h[0] * g.w[0];
    const int item = blockIdx.x;
    const int t = item / R, rcell = item - t * R;
    const int I = rcell / g.w[0], J = rcell % g.w[0];
    const int tid = threadIdx.x;
    for (int s = tid; s < TC::NNODE; s += blockDim.x) orow[s] = -1;
    for (int s = tid; s < TC::NPAR; s += blockDim.x) stop[s] = 1;
    if (tid == 0) { lcount[0] = 0; lcount[1] = 0; }
    lds_barrier();
    const float* part = reinterpret_cast<const float*>(a.S) + (int64_t)item * nchunk * TC::NSTAT;
    decide_and_emit<D, PERHEAD>(a, t, I, J, item, part, stat, stop, orow, lcount, inrm_l, nchunk);
}

// pass C: the chunk's channels of every emitted node, pooled from the leaves (k_node_apply's walk, one chunk of lanes per workgroup)
template <typename T, int VEC>
__global__ void __launch_bounds__(1024) k_wide_emit(const SpatialArgs a0, const BatchPtrs bp, int nchunk) {
    SpatialArgs a = a0;
    rebase(a, bp, blockIdx.y);
    const LevelDims& g = a0.dims;      // (the kernel argument: the level loops below index it at run time, a register copy would spill)
    const int D = g.n_level;
    const int R = g.h[0] * g.w[0];
    const int item = blockIdx.x / nchunk, chunk = blockIdx.x - item * nchunk;
    const int t = item / R;
    const int* list = a.rc_list + (int64_t)item * a.rc_stride;
    const int n = list[0] & 0xffff;
    const int HW = a.H * a.W;
    SpatialCtx cx;
    spatial_ctx_init<T>(cx, a, t, chunk * (int)blockDim.x + threadIdx.x, VEC);
    for (int k = 0; k < n; ++k) {
        const unsigned b = (unsigned)list[1 + k];
        const int y1 = b >> 24, x1 = (b >> 16) & 255, y2 = (b >> 8) & 255, x2 = b & 255;
        if (a.leaves_in_x && y2 - y1 == 1 && x2 - x1 == 1) continue;       // consumers read 1x1 rows from the input itself
        // the node is the cell, among the ancestors of leaf (y1, x1), whose box ends at (y2, x2)
        int ci = y1, cj = x1, lvl = D - 1;
        for (int l = D - 1; l >= 0; --l) {
            int hi_i = ci, hi_j = cj;
            for (int m = l; m < D - 1; ++m) {
                hi_i = child_start(hi_i, g.h[m + 1]) + child_count(hi_i, g.h[m + 1]) - 1;
                hi_j = child_start(hi_j, g.w[m + 1]) + child_count(hi_j, g.w[m + 1]) - 1;
            }
            lvl = l;
            if (hi_i + 1 == y2 && hi_j + 1 == x2) break;
            if (l > 0) { ci = parent_of(ci, g.h[l]); cj = parent_of(cj, g.w[l]); }
        }
        // (a store per depth: one pack merged over the four cases spilled in the 1-wide instantiation)
        const int64_t dst = (int64_t)(t * HW + y1 * a.W + x1) * a.C + cx.c0;
        switch (D - 1 - lvl) {
            case 0: if (cx.active) store_pack<T, VEC>(a.S, dst, AliasPool<T, VEC, 0>::run(cx, g, t, lvl, ci, cj)); break;
            case 1: { const Pack<T, VEC> v = AliasPool<T, VEC, 1>::run(cx, g, t, lvl, ci, cj); if (cx.active) store_pack<T, VEC>(a.S, dst, v); } break;
            case 2: { const Pack<T, VEC> v = AliasPool<T, VEC, 2>::run(cx, g, t, lvl, ci, cj); if (cx.active) store_pack<T, VEC>(a.S, dst, v); } break;
            default: { const Pack<T, VEC> v = AliasPool<T, VEC, 3>::run(cx, g, t, lvl, ci, cj); if (cx.active) store_pack<T, VEC>(a.S, dst, v); } break;   // a 4-level root cell
        }
    }
}

template <typename T, int VEC, bool PERHEAD>
static hipError_t launch_wide_vec(const SpatialArgs& a, const BatchPtrs& bp, int n_videos, int nt, int nchunk, hipStream_t stream) {
    const int items = a.T * a.dims.h[0] * a.dims.w[0];
    const dim3 ga(items * nchunk, n_videos), gb(items, n_videos);
    const int nwave = nt / kWave;
    if (nt > wide_max_lanes(a.dims.n_level) || nt % kWave) return hipErrorInvalidValue;
    switch (a.dims.n_level) {
#define STTM_WIDE_PASSES(BL, UL)                                                                                                  \
        hipLaunchKernelGGL((k_wide_stats<T, VEC, BL, UL, PERHEAD>), ga, dim3(nt), sizeof(float) * nwave * TreeConst<BL + UL>::NSTAT, \
                           stream, a, bp, nchunk);                                                                                 \
        hipLaunchKernelGGL((k_wide_decide<BL + UL, PERHEAD>), gb, dim3(256), 0, stream, a, bp, nchunk);                          \
        break
        case 1: STTM_WIDE_PASSES(1, 0);
        case 2: STTM_WIDE_PASSES(2, 0);
        case 3: STTM_WIDE_PASSES(3, 0);
        case 4: STTM_WIDE_PASSES(3, 1);
#undef STTM_WIDE_PASSES
        default: return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL((k_wide_emit<T, VEC>), ga, dim3(nt), 0, stream, a, bp, nchunk);
    return hipGetLastError();
}

// per-dtype entry point (spatial_wide_*.hip): vec = the row's pack width (no 32-byte packs), nt = lanes per chunk (a multiple of 64;
// at most wide_max_lanes(n_level))
template <typename T, bool PERHEAD>
hipError_t launch_spatial_wide_t(const SpatialArgs& a, const BatchPtrs& bp, int n_videos, int vec, int nt, int nchunk, hipStream_t stream) {
    using V = VecChoices<T>;
    if (vec == V::a) return launch_wide_vec<T, V::a, PERHEAD>(a, bp, n_videos, nt, nchunk, stream);
    if (vec == V::b) return launch_wide_vec<T, V::b, PERHEAD>(a, bp, n_videos, nt, nchunk, stream);
    if (vec == V::c) return launch_wide_vec<T, V::c, PERHEAD>(a, bp, n_videos, nt, nchunk, stream);
    return hipErrorInvalidValue;
}

}  // namespace sttm
