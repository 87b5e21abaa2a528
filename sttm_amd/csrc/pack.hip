// Ragged pack of the batched quadtree hook (sttm_pack_merged_batch, include/sttm_hip.h): B left-padded prompt rows, each with its
// video merged to N'_b rows by the batch entry point, become ONE compact left-padded block [B, Lout, C] plus the key mask, the
// position ids and every row's merged_token_1d_idx.
//   row b, column c, j = c - pad_out:   j < 0 zero | j < start  hidden[pad_in + j] | j < start + n  feat[j - start]
//                                       | else hidden[pad_in + j - n + length]
// A wave owns one output column at a time: its source is wave-uniform (three comparisons on scalar registers, no division), the
// lanes copy its row in PACK-byte words, four words in flight per lane.  Lane 0 also writes the column's mask word, its position
// ids and, on a merged column, idx = t * H * W + y1 * W + x1 from the row's tlbr (the arithmetic of the one-video idx_out).
// Bandwidth-bound: every valid row is read once and written once; the pad rows are only written.  Bytes are moved, never converted.
#include "sttm_kernels.h"

namespace sttm {

template <int PACK> struct PackWord;
template <> struct PackWord<16> { using type = uint4; };
template <> struct PackWord<8> { using type = uint2; };
template <> struct PackWord<4> { using type = uint32_t; };
template <> struct PackWord<2> { using type = uint16_t; };

constexpr int kPackWaves = 4;            // waves per workgroup
constexpr int kPackColsPerWave = 4;      // output columns per wave
constexpr int kPackUnroll = 4;           // words in flight per lane

template <int PACK>
__global__ void __launch_bounds__(kPackWaves * kWave) k_pack_merged(PackArgs a) {
    using W = typename PackWord<PACK>::type;
    const int r = blockIdx.y;
    const PackRow& d = a.rows[r];
    const int b = a.b0 + r;
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int c_end = min(a.Lout, (int)(blockIdx.x + 1) * kPackWaves * kPackColsPerWave);
    const char* hid = a.hidden + (int64_t)b * a.hid_stride_b;
    char* out_row = a.out + (int64_t)b * a.Lout * a.row_bytes;
    for (int c = blockIdx.x * kPackWaves * kPackColsPerWave + wave; c < c_end; c += kPackWaves) {
        const int j = c - d.pad_out;
        const char* src = nullptr;
        int col = 0;                                  // input column of the token (merged: the video's first + idx)
        int m = -1;                                   // merged row
        if (j >= 0) {
            if (j < d.start) {
                col = j;
                src = hid + (int64_t)(d.pad_in + j) * a.hid_stride_t;
            } else if (j < d.start + d.n) {
                m = j - d.start;
                src = d.feat + (int64_t)m * a.row_bytes;
            } else {
                col = j - d.n + d.length;
                src = hid + (int64_t)(d.pad_in + col) * a.hid_stride_t;
            }
        }
        W* dst = reinterpret_cast<W*>(out_row + (int64_t)c * a.row_bytes);
        if (src) {
            const W* s = reinterpret_cast<const W*>(src);
            for (int k0 = lane; k0 < a.packs; k0 += kPackUnroll * kWave) {
                W v[kPackUnroll];
#pragma unroll
                for (int u = 0; u < kPackUnroll; ++u)
                    if (k0 + u * kWave < a.packs) v[u] = s[k0 + u * kWave];
#pragma unroll
                for (int u = 0; u < kPackUnroll; ++u)
                    if (k0 + u * kWave < a.packs) dst[k0 + u * kWave] = v[u];
            }
        } else {
            const W z{};
            for (int k = lane; k < a.packs; k += kWave) dst[k] = z;
        }
        if (lane == 0) {
            const int64_t o = (int64_t)b * a.Lout + c;
            a.mask[o] = j >= 0 ? 1 : 0;
            if (m >= 0) {
                const int32_t* t = d.tlbr + (int64_t)m * 5;
                const int idx = t[0] * d.hw + t[1] * d.w + t[2];
                d.idx[m] = idx;
                // the merge kernels only emit cells of the grid; anything else reads the video's first id instead of
                // leaving the row
                col = d.start + ((unsigned)idx < (unsigned)d.length ? idx : 0);
            }
            if (a.pos_mode == STTM_PACK_POS_TRUNCATE) {
                a.pos_out[o] = j >= 0 ? a.pos_in[(int64_t)b * a.pos_stride_b + d.pad_in + j] : 1;
            } else if (a.pos_mode == STTM_PACK_POS_GATHER3) {
                for (int ax = 0; ax < 3; ++ax)
                    a.pos_out[(int64_t)ax * a.B * a.Lout + o] =
                        j >= 0 ? a.pos_in[ax * a.pos_stride_a + (int64_t)b * a.pos_stride_b + d.pad_in + col] : 1;
            }
        }
    }
}

hipError_t launch_pack_merged(const PackArgs& a, int n_rows, int pack_bytes, hipStream_t stream) {
    const int cols = kPackWaves * kPackColsPerWave;
    const dim3 grid((unsigned)((a.Lout + cols - 1) / cols), (unsigned)n_rows), block(kPackWaves * kWave);
    switch (pack_bytes) {
        case 16: hipLaunchKernelGGL(k_pack_merged<16>, grid, block, 0, stream, a); break;
        case 8: hipLaunchKernelGGL(k_pack_merged<8>, grid, block, 0, stream, a); break;
        case 4: hipLaunchKernelGGL(k_pack_merged<4>, grid, block, 0, stream, a); break;
        case 2: hipLaunchKernelGGL(k_pack_merged<2>, grid, block, 0, stream, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace sttm
