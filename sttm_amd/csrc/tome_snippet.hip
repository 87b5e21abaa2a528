// Per-frame / per-snippet ToMe: one iteration of tome_per_video's loop (tome_token_merger.py:143-149) over n_seg independent
// segments of n tokens each, all in the same four launches whatever n_seg is:
//   k_tsn_normalize   head-mean metric, unit rows; even / odd split by the token's index INSIDE its segment (n may be odd)
//   k_tsn_match       block-diagonal scores: a workgroup owns 128 a-rows of ONE segment and walks that segment's b-rows in tiles of
//                     128 with the running max / argmax in registers (v_mfma_f32_32x32x16 bf16 / f16; fp32 inputs as two fp16 planes,
//                     three plane products).  Every a-row has one owner, so the row maxima are combined in LDS and stored -- no
//                     atomics on global memory, no zeroed workspace.
//   k_tsn_rank        one workgroup per segment: ranking by counting in LDS (at most 512 keys), the per-destination source lists in
//                     rank order
//   k_tsn_merge       the size-weighted merge, one wave per output row; ids are global (segment * n + local id)
// A segment is a frame or a few frames (196 .. 784 tokens): the work per segment is tiny and there are many, so the path is bound by
// the bytes of x and by launches, not by the matrix pipe.  Same arithmetic as tome.hip (ties to the smaller index, 16-bit inputs round
// every intermediate to the input dtype); the cap on n is kTsnMaxTokens.
#include "tome_device.h"

namespace sttm {

constexpr int kTsnMaxTokens = STTM_TOME_SEGMENT_MAX_TOKENS;
constexpr int kTsnMaxHalf = (kTsnMaxTokens + 1) / 2;       // a-rows / b-rows of a segment at most

// ---------------------------------------------------------------------------------------------------
// normalise: one wave per token row.  T = float: two fp16 planes (h, l of 4096 v) per matrix, plane stride n_seg * rows;
// T = bf16 / f16: unit rows in the input dtype.  VEC > 1: one head, aligned rows (the production shapes).
// ---------------------------------------------------------------------------------------------------
template <typename T, int VEC>
__global__ void __launch_bounds__(256) k_tsn_normalize(const void* __restrict__ x_, int n_seg, int n, int C, int n_head, int D, int Dp,
                                                       uint16_t* __restrict__ ap, uint16_t* __restrict__ bp, int* __restrict__ bflag /*[n_seg * nb]*/) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const int na = (n + 1) / 2, nb = n / 2;
    const int total = n_seg * n;
    for (int row = blockIdx.x * nwave + wave; row < total; row += gridDim.x * nwave) {
        const int seg = row / n, l = row - seg * n;
        const bool odd = l & 1;
        const int64_t mrow = (int64_t)seg * (odd ? nb : na) + (l >> 1);
        uint16_t* out = (odd ? bp : ap) + mrow * Dp;
        // b-rows: is the unit row non-finite (tome_device.h: only possible with a norm of 0, Inf or NaN)?  Every b-row writes its flag,
        // so the flags need no zeroing; k_tsn_rank takes the segment's first flagged row.
        bool bad = false;
        if constexpr (std::is_same<T, float>::value) {
            const float* xr = reinterpret_cast<const float*>(x_) + (int64_t)row * C;
            uint16_t* hi = out;
            uint16_t* lo = hi + (int64_t)n_seg * (odd ? nb : na) * Dp;
            auto split = [&](float m, float nrm, uint16_t& h_out, uint16_t& l_out) {
                const float v = (m / nrm) * kSplitScale;                  // the reference's unit-row element, times 2^12 (exact)
                const _Float16 h = (_Float16)v;
                const _Float16 lw = (_Float16)(v - (float)h);             // v - h is exact in fp32
                h_out = __builtin_bit_cast(uint16_t, h);
                l_out = __builtin_bit_cast(uint16_t, lw);
            };
            if constexpr (VEC == 4) {
                float ss = 0.f;
                for (int d = lane * 4; d < D; d += 256) {
                    const float4 m = *reinterpret_cast<const float4*>(xr + d);
                    ss = fmaf(m.x, m.x, ss); ss = fmaf(m.y, m.y, ss); ss = fmaf(m.z, m.z, ss); ss = fmaf(m.w, m.w, ss);
                }
                ss = wave_sum(ss);
                const float nrm = sqrtf(ss);
                for (int d = lane * 4; d < D; d += 256) {
                    const float4 m = *reinterpret_cast<const float4*>(xr + d);
                    uint16_t h[4], lw[4];
                    split(m.x, nrm, h[0], lw[0]); split(m.y, nrm, h[1], lw[1]); split(m.z, nrm, h[2], lw[2]); split(m.w, nrm, h[3], lw[3]);
                    *reinterpret_cast<uint2*>(hi + d) = make_uint2((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16));
                    *reinterpret_cast<uint2*>(lo + d) = make_uint2((uint32_t)lw[0] | ((uint32_t)lw[1] << 16), (uint32_t)lw[2] | ((uint32_t)lw[3] << 16));
                }
                if (odd && tome_norm_degenerate(nrm)) {
                    for (int d = lane * 4; d < D; d += 256) {
                        const float4 m = *reinterpret_cast<const float4*>(xr + d);
                        bad |= tome_unit_nonfinite(m.x, nrm) || tome_unit_nonfinite(m.y, nrm) || tome_unit_nonfinite(m.z, nrm) || tome_unit_nonfinite(m.w, nrm);
                    }
                }
            } else {
                auto metric = [&](int d) {
                    if (n_head == 1) return xr[d];
                    float s = 0.f;
                    for (int h = 0; h < n_head; ++h) s += xr[h * D + d];
                    return s / (float)n_head;
                };
                float ss = 0.f;
                for (int d = lane; d < D; d += 64) { const float m = metric(d); ss = fmaf(m, m, ss); }
                ss = wave_sum(ss);
                const float nrm = sqrtf(ss);
                for (int d = lane; d < D; d += 64) split(metric(d), nrm, hi[d], lo[d]);
                if (odd && tome_norm_degenerate(nrm)) {
                    for (int d = lane; d < D; d += 64) bad |= tome_unit_nonfinite(metric(d), nrm);
                }
            }
            for (int d = D + lane; d < Dp; d += 64) { hi[d] = 0; lo[d] = 0; }
        } else {
            if constexpr (VEC == 8) {
                constexpr int MAXCH = 8;                     // chunks of 512 elements: D <= 4096
                Pack<T, 8> v[MAXCH];
                float ss = 0.f;
#pragma unroll
                for (int i = 0; i < MAXCH; ++i) {
                    const int d = (i * 64 + lane) * 8;
                    if (d < D) {
                        v[i] = load_pack<T, 8>(x_, (int64_t)row * C + d);
#pragma unroll
                        for (int e = 0; e < 8; ++e) { const float m = v[i].get(e); ss = fmaf(m, m, ss); }
                    }
                }
                ss = wave_sum(ss);
                const float nrm = tome_round<T>(sqrtf(ss));
#pragma unroll
                for (int i = 0; i < MAXCH; ++i) {
                    const int d = (i * 64 + lane) * 8;
                    if (d < D) {
                        Pack<T, 8> o;
                        const Pack<T, 8> in = v[i];
                        pack_fill<T, 8>(o, [&](int e) { return in.get(e) / nrm; });
                        store_pack<T, 8>(out, d, o);
                    }
                }
                if (odd && tome_norm_degenerate(nrm)) {
#pragma unroll
                    for (int i = 0; i < MAXCH; ++i) {
                        if ((i * 64 + lane) * 8 < D) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) bad |= tome_unit_nonfinite(v[i].get(e), nrm);
                        }
                    }
                }
            } else {
                float ss = 0.f;
                for (int d = lane; d < D; d += 64) {
                    float m;
                    if (n_head == 1) {
                        m = tome_ld<T>(x_, (int64_t)row * C + d);
                    } else {
                        float s = 0.f;
                        for (int h = 0; h < n_head; ++h) s += tome_ld<T>(x_, (int64_t)row * C + h * D + d);
                        m = tome_round<T>(s / (float)n_head);
                    }
                    tome_st<T>(out, d, m);
                    ss = fmaf(m, m, ss);
                }
                ss = wave_sum(ss);
                const float nrm = tome_round<T>(sqrtf(ss));
                for (int d = lane; d < D; d += 64) tome_st<T>(out, d, tome_ld<T>(out, d) / nrm);
                if (odd && tome_norm_degenerate(nrm)) {
                    for (int d = lane; d < D; d += 64) bad |= tome_unit_nonfinite(tome_ld<T>(out, d), nrm);
                }
            }
            for (int d = D + lane; d < Dp; d += 64) out[d] = 0;
        }
        if (odd) {
            const bool any = __builtin_amdgcn_ballot_w64(bad) != 0ull;
            if (lane == 0) bflag[mrow] = any ? 1 : 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// match: workgroup = (segment, tile of 128 a-rows); four waves of 64 (j) x 64 (i), the transposed tile D[j][i] = b_j . a_i of
// tome.hip's 128-tile kernels (a lane owns a-rows, its candidates come in ascending j).  NP = 2: fp32 inputs as two fp16 planes,
// TERMS plane products (T = f16_t); NP = 1: 16-bit inputs of type T, scores rounded to T before they are compared.
// ---------------------------------------------------------------------------------------------------
constexpr int TSN_T = 128;       // tile side
constexpr int TSN_K = 32;        // k per LDS stage
template <typename T, int NP, int TERMS>
__global__ void __launch_bounds__(256, 2) k_tsn_match(const uint16_t* __restrict__ ap, const uint16_t* __restrict__ bp, int n_seg,
                                                       int na, int nb, int D, int itiles, unsigned long long* __restrict__ best /*[n_seg * na]*/) {
    static_assert((NP == 2 && (TERMS == 3 || TERMS == 4)) || (NP == 1 && TERMS == 1), "plane / term combination");
    constexpr int NT = 256, QI = 2;
    constexpr int LD = TSN_K + 8;               // LDS row: 32 elements + 16 bytes (ds_read_b128 groups hit distinct 4-bank groups)
    constexpr int CPR = TSN_K / 8;              // 16-byte chunks per row and stage
    constexpr int NLD = NP * TSN_T * CPR / NT;  // 16-byte loads per thread, matrix and stage
    __shared__ __attribute__((aligned(16))) uint16_t As[NP * TSN_T * LD];      // [plane][row][LD]
    __shared__ __attribute__((aligned(16))) uint16_t Bs[NP * TSN_T * LD];
    __shared__ unsigned long long red[TSN_T];
    typedef typename TomeMfma<T>::vec vec;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave & 1, wj = wave >> 1;
    const int seg = blockIdx.x / itiles, itile = blockIdx.x - seg * itiles;
    const int i0 = itile * TSN_T;
    const int64_t a_plane = (int64_t)n_seg * na, b_plane = (int64_t)n_seg * nb;
    const int64_t a_base = (int64_t)seg * na, b_base = (int64_t)seg * nb;
    const int jtiles = (nb + TSN_T - 1) / TSN_T;
    float bestv[QI];
    int bestj[QI];
#pragma unroll
    for (int q = 0; q < QI; ++q) { bestv[q] = -INFINITY; bestj[q] = 0x7fffffff; }
    if (tid < TSN_T) red[tid] = 0ull;
    const int lcol = lane & 31, lhalf = lane >> 5;
    tome_u32x4 ra[NLD], rb[NLD];
    // rows are zero-padded to a multiple of 64 by k_tsn_normalize, so a stage needs no k bound; rows past the segment's end are
    // clamped to its last row: their scores are computed and ignored (i < na at the store, j < nb in the running max)
    auto fetch = [&](int j0, int k0) {
#pragma unroll
        for (int c = 0; c < NLD; ++c) {
            const int id = c * NT + tid, plane = id / (TSN_T * CPR), rem = id % (TSN_T * CPR), row = rem / CPR, ch = rem % CPR;
            const int ri = min(i0 + row, na - 1), rj = min(j0 + row, nb - 1);
            ra[c] = *reinterpret_cast<const tome_u32x4*>(ap + (plane * a_plane + a_base + ri) * D + k0 + ch * 8);
            rb[c] = *reinterpret_cast<const tome_u32x4*>(bp + (plane * b_plane + b_base + rj) * D + k0 + ch * 8);
        }
    };
    fetch(0, 0);
    for (int jt = 0; jt < jtiles; ++jt) {
        const int j0 = jt * TSN_T;
        f32x16_t acc[2][QI];
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = 0; q < QI; ++q)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[p][q][e] = 0.f;
        for (int k0 = 0; k0 < D; k0 += TSN_K) {
            __syncthreads();          // previous stage fully consumed
#pragma unroll
            for (int c = 0; c < NLD; ++c) {
                const int id = c * NT + tid, plane = id / (TSN_T * CPR), rem = id % (TSN_T * CPR), row = rem / CPR, ch = rem % CPR;
                *reinterpret_cast<tome_u32x4*>(As + (plane * TSN_T + row) * LD + ch * 8) = ra[c];
                *reinterpret_cast<tome_u32x4*>(Bs + (plane * TSN_T + row) * LD + ch * 8) = rb[c];
            }
            __syncthreads();
            if (k0 + TSN_K < D) fetch(j0, k0 + TSN_K);
            else if (jt + 1 < jtiles) fetch(j0 + TSN_T, 0);
#pragma unroll
            for (int ks = 0; ks < TSN_K; ks += 16) {
                vec fb[2][NP], fa[QI][NP];      // [subtile][plane: 0 = h, 1 = l]
#pragma unroll
                for (int pl = 0; pl < NP; ++pl) {
#pragma unroll
                    for (int p = 0; p < 2; ++p)
                        fb[p][pl] = *reinterpret_cast<const vec*>(Bs + (pl * TSN_T + wj * 64 + p * 32 + lcol) * LD + ks + lhalf * 8);
#pragma unroll
                    for (int q = 0; q < QI; ++q)
                        fa[q][pl] = *reinterpret_cast<const vec*>(As + (pl * TSN_T + wi * 64 + q * 32 + lcol) * LD + ks + lhalf * 8);
                }
                if constexpr (NP == 2) {
                    // terms outermost: consecutive MFMAs write different accumulators
#pragma unroll
                    for (int term = 4 - TERMS; term < 4; ++term) {
                        const int pb = term == 0 || term == 1, pa = term == 0 || term == 2;    // l.l, l.h, h.l, h.h
#pragma unroll
                        for (int p = 0; p < 2; ++p)
#pragma unroll
                            for (int q = 0; q < QI; ++q) acc[p][q] = TomeMfma<T>::run(fb[p][pb], fa[q][pa], acc[p][q]);
                    }
                } else {
#pragma unroll
                    for (int p = 0; p < 2; ++p)
#pragma unroll
                        for (int q = 0; q < QI; ++q) acc[p][q] = TomeMfma<T>::run(fb[p][0], fa[q][0], acc[p][q]);
                }
            }
        }
        // NP = 2: on the scaled scores (the factor 2^-24 is applied once, at the end); NP = 1: the score tensor of the reference has
        // the input dtype, round before comparing (ties -> smaller j)
        if constexpr (NP == 2)
            tome_running_max<QI>(acc, bestv, bestj, j0 + wj * 64 + 4 * lhalf, nb, j0 + TSN_T <= nb, [](float v) { return v; });
        else
            tome_running_max<QI>(acc, bestv, bestj, j0 + wj * 64 + 4 * lhalf, nb, j0 + TSN_T <= nb, [](float v) { return tome_round<T>(v); });
    }
    // combine the two lane halves and the two j-waves of an a-row in LDS (a row without a finite score keeps 0, like tome.hip)
    __syncthreads();
#pragma unroll
    for (int q = 0; q < QI; ++q)
        if (bestj[q] != 0x7fffffff) atomicMax(&red[wi * 64 + q * 32 + lcol], pack_score(NP == 2 ? bestv[q] * kSplitUnscale : bestv[q], bestj[q]));
    __syncthreads();
    if (tid < TSN_T && i0 + tid < na) best[a_base + i0 + tid] = red[tid];
}

// ---------------------------------------------------------------------------------------------------
// rank + lists: one workgroup per segment.  rank_i = #{ j : key_j > key_i } on the distinct 64-bit keys of tome_rank_key
// (argsort(node_max, descending), ties to the smaller index); the r best a-rows are sources, grouped per destination b-row in
// rank order:  order [n_seg][na] a-rows by rank, off [n_seg][nb + 1] list starts, lists [n_seg][na] a-rows (r entries used).
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_tsn_rank(const unsigned long long* __restrict__ best, const int* __restrict__ bflag, int na, int nb, int r,
                                                  int* __restrict__ order, int* __restrict__ off, int* __restrict__ lists) {
    __shared__ unsigned long long key[kTsnMaxHalf];
    __shared__ int ord[kTsnMaxHalf], dst[kTsnMaxHalf];
    __shared__ __attribute__((aligned(16))) int dk[kTsnMaxHalf + 4];      // destination of the source of rank k
    __shared__ int cnt[kTsnMaxHalf + 1];
    __shared__ unsigned pw_sh;                 // 0xffffffff - (the segment's first poisoned b-row), 0 on clean inputs (tome_device.h)
    const int tid = threadIdx.x, seg = blockIdx.x;
    const int64_t a_base = (int64_t)seg * na;
    if (tid == 0) pw_sh = 0u;
    __syncthreads();
    for (int j = tid; j < nb; j += 256)
        if (bflag[(int64_t)seg * nb + j]) atomicMax(&pw_sh, 0xffffffffu - (unsigned)j);
    __syncthreads();
    const unsigned pw = pw_sh;
    for (int i = tid; i < na; i += 256) {
        const unsigned long long b = tome_poisoned_best(best[a_base + i], pw);
        key[i] = tome_rank_key(b, i);
        dst[i] = b ? (int)(0xffffffffu - (unsigned)(b & 0xffffffffu)) : 0;
    }
    for (int j = tid; j <= nb; j += 256) cnt[j] = 0;
    __syncthreads();
    for (int i = tid; i < na; i += 256) {
        const unsigned long long ki = key[i];
        int c = 0;
        for (int q = 0; q < na; ++q) c += key[q] > ki ? 1 : 0;        // LDS broadcast reads
        ord[c] = i;
    }
    __syncthreads();
    for (int k = tid; k < na; k += 256) order[a_base + k] = ord[k];
    const int r4 = (r + 3) & ~3;
    for (int k = tid; k < r4; k += 256) dk[k] = k < r ? dst[ord[k]] : -1;
    __syncthreads();
    int pos[(kTsnMaxHalf + 255) / 256];
#pragma unroll
    for (int u = 0; u < (kTsnMaxHalf + 255) / 256; ++u) {
        const int k = tid + u * 256;
        pos[u] = 0;
        if (k < r) {
            const int d = dk[k];
            int c = 0;
            for (int q = 0; q < k; q += 4) {                            // sources of the same destination with a better rank
                const int4 v = *reinterpret_cast<const int4*>(dk + q);
                c += (v.x == d) + (v.y == d && q + 1 < k) + (v.z == d && q + 2 < k) + (v.w == d && q + 3 < k);
            }
            pos[u] = c;
            atomicAdd(&cnt[d], 1);
        }
    }
    __syncthreads();
    if (tid == 0) {                                                     // exclusive scan of at most 513 counts
        int run = 0;
        for (int j = 0; j <= nb; ++j) { const int c = cnt[j]; cnt[j] = run; run += c; }
    }
    __syncthreads();
    for (int j = tid; j <= nb; j += 256) off[(int64_t)seg * (nb + 1) + j] = cnt[j];
#pragma unroll
    for (int u = 0; u < (kTsnMaxHalf + 255) / 256; ++u) {
        const int k = tid + u * 256;
        if (k < r) lists[a_base + cnt[dk[k]] + pos[u]] = ord[k];
    }
}

// ---------------------------------------------------------------------------------------------------
// merge: one wave per output row.  Per segment, rows [0, na - r): unmerged a-tokens in rank order; rows [na - r, n - r): b-tokens
// with their sources folded in, in rank order.  Arithmetic of k_tome_merge (tome.hip): every tensor of the reference is rounded to
// the input dtype T -- x * size, the scatter-added sum (accumulated in fp32, rounded once), the sum of sizes, the quotient.
// ---------------------------------------------------------------------------------------------------
template <typename T, int VEC>
__global__ void __launch_bounds__(256) k_tsn_merge(const void* __restrict__ x, const float* __restrict__ size, const int64_t* __restrict__ idx,
                                                   int n_seg, int n, int C, int r, const int* __restrict__ order, const int* __restrict__ off,
                                                   const int* __restrict__ lists, void* __restrict__ x_out, float* __restrict__ size_out,
                                                   int64_t* __restrict__ idx_out) {
#pragma clang fp contract(off)      // x*size is rounded before it is added, like the reference's mul then scatter-add

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const int na = (n + 1) / 2, nb = n / 2, n_out = n - r;
    const int total = n_seg * n_out;
    constexpr int NCH = VEC >= 8 ? 2 : 4;   // chunks of 64 * VEC channels handled together
    for (int row = blockIdx.x * nwave + wave; row < total; row += gridDim.x * nwave) {
        const int seg = row / n_out, lr = row - seg * n_out;
        const int64_t t0 = (int64_t)seg * n, a_base = (int64_t)seg * na;
        if (lr < na - r) {
            const int64_t tok = t0 + 2 * order[a_base + r + lr];      // unmerged a-token: (x*size)/size
            const float s = size ? size[tok] : 1.f;
            for (int c0 = 0; c0 < C; c0 += NCH * 64 * VEC) {
                float v[NCH][VEC];
#pragma unroll
                for (int u = 0; u < NCH; ++u) {
                    const int c = c0 + (u * 64 + lane) * VEC;
                    if (c < C) tome_ld_vec<T, VEC>(x, tok * C + c, v[u]);
                }
#pragma unroll
                for (int u = 0; u < NCH; ++u) {
                    const int c = c0 + (u * 64 + lane) * VEC;
                    if (c < C) {
#pragma unroll
                        for (int e = 0; e < VEC; ++e) v[u][e] = tome_round<T>(v[u][e] * s) / s;
                        tome_st_vec<T, VEC>(x_out, (int64_t)row * C + c, v[u]);
                    }
                }
            }
            if (lane == 0) { size_out[row] = s; idx_out[row] = idx ? idx[tok] : tok; }
            continue;
        }
        const int j = lr - (na - r);
        const int64_t tok = t0 + 2 * j + 1;
        const int* lst = lists + a_base;
        const int o = off[(int64_t)seg * (nb + 1) + j], cnt = off[(int64_t)seg * (nb + 1) + j + 1] - o;
        const float sb = size ? size[tok] : 1.f;
        float stot = sb;
        for (int m = 0; m < cnt; ++m) {
            const int64_t atok = t0 + 2 * lst[o + m];
            stot = stot + (size ? size[atok] : 1.f);
        }
        stot = tome_round<T>(stot);
        for (int c0 = 0; c0 < C; c0 += NCH * 64 * VEC) {
            float acc[NCH][VEC], xa[NCH][VEC];
#pragma unroll
            for (int u = 0; u < NCH; ++u) {
                const int c = c0 + (u * 64 + lane) * VEC;
                if (c < C) tome_ld_vec<T, VEC>(x, tok * C + c, acc[u]);
            }
#pragma unroll
            for (int u = 0; u < NCH; ++u)
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[u][e] = tome_round<T>(acc[u][e] * sb);
            for (int m = 0; m < cnt; ++m) {
                const int64_t atok = t0 + 2 * lst[o + m];
                const float sa = size ? size[atok] : 1.f;
#pragma unroll
                for (int u = 0; u < NCH; ++u) {
                    const int c = c0 + (u * 64 + lane) * VEC;
                    if (c < C) tome_ld_vec<T, VEC>(x, atok * C + c, xa[u]);
                }
#pragma unroll
                for (int u = 0; u < NCH; ++u) {
                    const int c = c0 + (u * 64 + lane) * VEC;
                    if (c < C) {
#pragma unroll
                        for (int e = 0; e < VEC; ++e) acc[u][e] = acc[u][e] + tome_round<T>(xa[u][e] * sa);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < NCH; ++u) {
                const int c = c0 + (u * 64 + lane) * VEC;
                if (c < C) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) acc[u][e] = tome_round<T>(acc[u][e]) / stot;
                    tome_st_vec<T, VEC>(x_out, (int64_t)row * C + c, acc[u]);
                }
            }
        }
        if (lane == 0) { size_out[row] = stot; idx_out[row] = idx ? idx[tok] : tok; }
    }
}

static inline size_t tsn_al(size_t v) { return (v + 255) / 256 * 256; }

int tome_segments_plan(int n_seg, int n, int C, int n_head, TomeSegPlan* p) {
    if (n_seg < 1 || n < 2 || C < 1 || n_head < 1 || C % n_head) return STTM_ERR_ARG;
    if (n > kTsnMaxTokens) return STTM_ERR_UNSUPPORTED;
    if ((long long)n_seg * n > (1ll << 28)) return STTM_ERR_UNSUPPORTED;      // row numbers are 32-bit
    p->na = (n + 1) / 2; p->nb = n / 2; p->D = C / n_head;
    p->Dp = (p->D + 63) / 64 * 64;
    size_t o = 0;
    p->off_a = o; o = tsn_al(o + (size_t)n_seg * p->na * p->Dp * 4);          // two 16-bit planes at most
    p->off_b = o; o = tsn_al(o + (size_t)n_seg * p->nb * p->Dp * 4);
    p->off_best = o; o = tsn_al(o + (size_t)n_seg * p->na * 8);
    p->off_order = o; o = tsn_al(o + (size_t)n_seg * p->na * 4);
    p->off_off = o; o = tsn_al(o + (size_t)n_seg * (p->nb + 1) * 4);
    p->off_lists = o; o = tsn_al(o + (size_t)n_seg * p->na * 4);
    p->off_bflag = o; o = tsn_al(o + (size_t)n_seg * (p->nb > 0 ? p->nb : 1) * 4);
    p->total = o;
    return STTM_OK;
}

hipError_t launch_tome_segments(const void* x, const float* size, const int64_t* idx, int n_seg, int n, int C, int n_head, int r, int dtype,
                                const TomeSegPlan& p, void* workspace, void* x_out, float* size_out, int64_t* idx_out, hipStream_t stream) {
    char* ws = reinterpret_cast<char*>(workspace);
    uint16_t* ap = reinterpret_cast<uint16_t*>(ws + p.off_a);
    uint16_t* bp = reinterpret_cast<uint16_t*>(ws + p.off_b);
    unsigned long long* best = reinterpret_cast<unsigned long long*>(ws + p.off_best);
    int* order = reinterpret_cast<int*>(ws + p.off_order);
    int* off = reinterpret_cast<int*>(ws + p.off_off);
    int* lists = reinterpret_cast<int*>(ws + p.off_lists);
    int* bflag = reinterpret_cast<int*>(ws + p.off_bflag);
    const long long rows = (long long)n_seg * n;
    const int ngrid = (int)((rows + 3) / 4 > 8192 ? 8192 : (rows + 3) / 4);
    const int itiles = (p.na + TSN_T - 1) / TSN_T;
    const bool al16 = reinterpret_cast<uintptr_t>(x) % 16 == 0;
    if (dtype == STTM_F32) {
        if (n_head == 1 && C % 4 == 0 && al16)
            hipLaunchKernelGGL((k_tsn_normalize<float, 4>), dim3(ngrid), dim3(256), 0, stream, x, n_seg, n, C, n_head, p.D, p.Dp, ap, bp, bflag);
        else
            hipLaunchKernelGGL((k_tsn_normalize<float, 1>), dim3(ngrid), dim3(256), 0, stream, x, n_seg, n, C, n_head, p.D, p.Dp, ap, bp, bflag);
        // three plane products (without l.l), the default of the per-clip path ("tome_split" = 2)
        hipLaunchKernelGGL((k_tsn_match<f16_t, 2, 3>), dim3(n_seg * itiles), dim3(256), 0, stream, ap, bp, n_seg, p.na, p.nb, p.Dp, itiles, best);
    } else {
#define STTM_TSN_16(TT)                                                                                                                   \
        do {                                                                                                                              \
            if (n_head == 1 && C % 8 == 0 && C <= 4096 && al16)                                                                           \
                hipLaunchKernelGGL((k_tsn_normalize<TT, 8>), dim3(ngrid), dim3(256), 0, stream, x, n_seg, n, C, n_head, p.D, p.Dp, ap, bp, bflag); \
            else                                                                                                                          \
                hipLaunchKernelGGL((k_tsn_normalize<TT, 1>), dim3(ngrid), dim3(256), 0, stream, x, n_seg, n, C, n_head, p.D, p.Dp, ap, bp, bflag); \
            hipLaunchKernelGGL((k_tsn_match<TT, 1, 1>), dim3(n_seg * itiles), dim3(256), 0, stream, ap, bp, n_seg, p.na, p.nb, p.Dp, itiles, best); \
        } while (0)
        if (dtype == STTM_BF16) STTM_TSN_16(bf16_t); else STTM_TSN_16(f16_t);
#undef STTM_TSN_16
    }
    hipLaunchKernelGGL(k_tsn_rank, dim3(n_seg), dim3(256), 0, stream, best, bflag, p.na, p.nb, r, order, off, lists);
    {
        const long long orows = (long long)n_seg * (n - r);
        const int grid = (int)((orows + 3) / 4 > 8192 ? 8192 : (orows + 3) / 4);
#define STTM_TSN_MERGE(TT, VV) hipLaunchKernelGGL((k_tsn_merge<TT, VV>), dim3(grid), dim3(256), 0, stream, x, size, idx, n_seg, n, C, r, order, off, lists, x_out, size_out, idx_out)
        const size_t eb = dtype == STTM_F32 ? 4 : 2;
        const bool v4 = C % 4 == 0 && reinterpret_cast<uintptr_t>(x) % (4 * eb) == 0 && reinterpret_cast<uintptr_t>(x_out) % (4 * eb) == 0;
        const bool v8 = C % 8 == 0 && al16 && reinterpret_cast<uintptr_t>(x_out) % 16 == 0;
        if (dtype == STTM_F32) { if (v4) STTM_TSN_MERGE(float, 4); else STTM_TSN_MERGE(float, 1); }
        else if (dtype == STTM_BF16) { if (v8) STTM_TSN_MERGE(bf16_t, 8); else if (v4) STTM_TSN_MERGE(bf16_t, 4); else STTM_TSN_MERGE(bf16_t, 1); }
        else { if (v8) STTM_TSN_MERGE(f16_t, 8); else if (v4) STTM_TSN_MERGE(f16_t, 4); else STTM_TSN_MERGE(f16_t, 1); }
#undef STTM_TSN_MERGE
    }
    return hipGetLastError();
}

}  // namespace sttm
