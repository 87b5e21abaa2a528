// Token-to-merged-row map of a finished quadtree merge (sttm_quadtree_token_map, include/sttm_hip.h).
//
// The map is a second consumer of the tables sttm_quadtree_apply reads -- "the merge that ran last on this stream with this
// workspace": meta (node boxes by origin row), lab_row (origin row of a node's representative, possibly in an earlier frame),
// gcnt (> 0 marks a survivor) and frame_cnt (survivors per frame).
//   k_survivor_rows    origin row of a survivor -> its row of feat_out: sum of frame_cnt[0 .. t) + its rank among the frame's survivors
//                      in row order, the numbering of k_group_mean (temporal_merge.hip), so the map cannot drift from the features.
//   k_paint_token_map  one wave per origin row; the wave of a node walks the node's box and writes, for every leaf, the output row of
//                      the node's representative and (optionally) the node's origin row.  The boxes tile every frame exactly once, so
//                      painting from the node side needs no pyramid geometry.
// A representative can sit in another frame than its member, so the two passes are TWO launches; there is no grid barrier.
//
// Where the intermediate table lives: in token_to_out itself.  k_survivor_rows writes entry r for every survivor origin row r (the
// other entries are not read); k_paint_token_map reads entry lab_row[origin] and overwrites every leaf.  That is safe because a
// representative is a fixed point of the labels (lab_row[r] == r for a survivor, the label stage stops on rep == rep[rep]): the only
// wave that writes a survivor's origin leaf is the wave of the survivor's own node, and it writes the value the entry already
// holds.  No entry that another wave reads ever changes its value.
// No atomics, no scratch, no host synchronisation.  Every index read from a table is range-checked before it is used as an address.
#include "sttm_kernels.h"

namespace sttm {

constexpr int kScanThreads = 1024;       // rows per scan chunk of k_survivor_rows (LDS: one counter per wave, whatever H * W is)
constexpr int kScanWaves = kScanThreads / kWave;

__global__ void __launch_bounds__(kScanThreads) k_survivor_rows(const int32_t* __restrict__ gcnt, const int32_t* __restrict__ frame_cnt,
                                                                int HW, int32_t* __restrict__ out_row) {
    __shared__ int wcnt[2][kScanWaves];
    const int t = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // rows before this frame
    int row0 = 0;
    for (int f = threadIdx.x; f < t; f += kScanThreads) row0 += frame_cnt[f];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) row0 += __shfl_xor(row0, o);
    if (lane == 0) wcnt[0][wave] = row0;
    __syncthreads();
    row0 = 0;
#pragma unroll
    for (int w = 0; w < kScanWaves; ++w) row0 += wcnt[0][w];
    const unsigned long long lt = (1ull << lane) - 1ull;
    int run = row0, buf = 1;
    for (int base = 0; base < HW; base += kScanThreads, buf ^= 1) {       // (two counter sets: one barrier per chunk)
        const int p = base + (int)threadIdx.x;
        const bool alive = p < HW && gcnt[(size_t)t * HW + p] > 0;
        const unsigned long long m = __ballot(alive);
        if (lane == 0) wcnt[buf][wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kScanWaves; ++w) {
            const int c = wcnt[buf][w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (alive) out_row[(size_t)t * HW + p] = run + before + __popcll(m & lt);
        run += total;
    }
}

constexpr int kPaintWaves = 4;

__global__ void __launch_bounds__(kPaintWaves * kWave) k_paint_token_map(const uint32_t* __restrict__ meta, const int32_t* __restrict__ lab_row,
                                                                         int N, int H, int W, int32_t* token_to_out, int32_t* token_to_node) {
    const int lane = threadIdx.x & 63;
    const int origin = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kPaintWaves + (threadIdx.x >> 6)));
    if (origin >= N) return;
    const uint32_t m = meta[origin];
    if (m == 0) return;
    const int HW = H * W;
    const int t = origin / HW, p = origin - t * HW;
    const int y1 = p / W, x1 = p - y1 * W;
    const int y2 = (int)(m >> 16), x2 = (int)(m & 0xffffu);
    if (y2 <= y1 || x2 <= x1 || y2 > H || x2 > W) return;              // not a box of this grid: nothing is written
    const int rep = lab_row[origin];
    const int v = (unsigned)rep < (unsigned)N ? token_to_out[rep] : -1;
    const int bw = x2 - x1, area = (y2 - y1) * bw;
    int32_t* o = token_to_out + (size_t)t * HW;
    int32_t* n = token_to_node ? token_to_node + (size_t)t * HW : nullptr;
    for (int i = lane; i < area; i += kWave) {
        const int dy = i / bw, dx = i - dy * bw;
        const int leaf = (y1 + dy) * W + x1 + dx;
        o[leaf] = v;
        if (n) n[leaf] = origin;
    }
}

hipError_t launch_token_map(const uint32_t* meta, const int32_t* lab_row, const int32_t* gcnt, const int32_t* frame_cnt, int T, int H, int W,
                            int32_t* token_to_out, int32_t* token_to_node, hipStream_t stream) {
    const int N = T * H * W;
    hipLaunchKernelGGL(k_survivor_rows, dim3((unsigned)T), dim3(kScanThreads), 0, stream, gcnt, frame_cnt, H * W, token_to_out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_paint_token_map, dim3((unsigned)((N + kPaintWaves - 1) / kPaintWaves)), dim3(kPaintWaves * kWave), 0, stream,
                       meta, lab_row, N, H, W, token_to_out, token_to_node);
    return hipGetLastError();
}

}  // namespace sttm
