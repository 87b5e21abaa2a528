// DyCoke stage 2 at decode time (batch 1, one query token): replaces what token_merging_monkey_patch/dycoke_attn_monkey_patch.py of
// the reference does on every generated token with an eager layer, a host list and two gathers of the whole cache per layer.
//
//   scores    (:80, `attn[1].mean(1)[0, -1]` of the eager layer dycoke_l - 1, :410-411)
//             k_dec_logits   one workgroup per (tile of K rows, KV head): the scaled logits of the tile for the query heads of the
//                            group (a K row is read once), written to the workspace with the tile's max and sum of exponentials
//             k_dec_score    combines the tile statistics per head, then score[j] = mean over heads of exp(l - M) / S, float32
//   select    (:62-77)  k_dec_select, one workgroup: radix select of the num_keep-th largest score of the window on the float bits
//             (four 8-bit passes; scores are non-negative, so the bit pattern orders them), then an ordered compaction: everything
//             above the threshold plus the first `need` entries equal to it, ascending by index.  The keep list stays on the device.
//   gathered  (:54-60 + the attention that follows)
//             k_dec_gathered one workgroup per (tile of keep entries, KV head): K and V rows read in place through `keep`, all loads
//                            of the tile in flight at once, tile-local softmax, partial (max, sum, p.V) per query head
//             k_dec_combine  one workgroup per query head merges the partials and writes the row in the model dtype
//
// A row of D elements is covered by D * sizeof(T) / 16 lanes with one 16-byte load each; a tile is 256 / that many lane groups times
// four rows.  Everything accumulates in float32.  No kernel uses scratch, none synchronises with the host.
#include <math.h>

#include "sttm_kernels.h"

namespace sttm {

constexpr int kDecThreads = 256;
constexpr int kDecRpg = 4;        // rows per lane group and tile
constexpr int kDecGmax = 8;       // query heads of one KV head handled per sweep (more heads: further sweeps over the same registers)

template <typename T, int D> struct DecTile {
    static constexpr int EPL = 16 / TypeInfo<T>::bytes;    // elements per lane
    static constexpr int LPR = D / EPL;                    // lanes per row
    static constexpr int GROUPS = kDecThreads / LPR;
    static constexpr int ROWS = GROUPS * kDecRpg;          // 32 (f32, 128) .. 128 (16-bit, 64)
};

template <typename T> __device__ __forceinline__ void dec_unpack(const uint4& u, float* f);
template <> __device__ __forceinline__ void dec_unpack<float>(const uint4& u, float* f) {
    f[0] = __uint_as_float(u.x); f[1] = __uint_as_float(u.y); f[2] = __uint_as_float(u.z); f[3] = __uint_as_float(u.w);
}
template <> __device__ __forceinline__ void dec_unpack<bf16_t>(const uint4& u, float* f) {
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[2 * i] = __uint_as_float(w[i] << 16); f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
}
template <> __device__ __forceinline__ void dec_unpack<f16_t>(const uint4& u, float* f) {
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[2 * i] = f16_bits_to_float(w[i] & 0xffffu); f[2 * i + 1] = f16_bits_to_float(w[i] >> 16); }
}

template <int CTRL> __device__ __forceinline__ float dec_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
// sum over the LPR (8, 16 or 32) consecutive lanes of a row; every lane of the group gets it
template <int LPR> __device__ __forceinline__ float dec_group_sum(float v) {
    v += dec_dpp<0xB1>(v);                         // quad_perm [1, 0, 3, 2]
    v += dec_dpp<0x4E>(v);                         // quad_perm [2, 3, 0, 1]
    v += dec_dpp<0x141>(v);                        // row_half_mirror
    if constexpr (LPR >= 16) v += dec_dpp<0x140>(v);   // row_mirror
    if constexpr (LPR >= 32) v += __shfl_xor(v, 16, 64);
    return v;
}
__device__ __forceinline__ float dec_wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

struct DecArgs {
    const void* q; int64_t q_sh;                  // [Hq, D], head stride in elements
    const void* k; int64_t k_sh, k_sl;            // [Hkv, Lk, D], head / row strides in elements
    const void* v; int64_t v_sh, v_sl;
    int Hq, Hkv, Lk;
    float scale;
    const int32_t* keep; int n_keep;
    float* logits;                                // scores: [Hq, Lk]
    float* part;                                  // [tiles, Hq, 2] max and sum of exponentials of a tile
    float* pacc;                                  // gathered: [tiles, Hq, D]
};

// The scaled logits of the tile's rows for query heads [g0, g0 + gn) of KV head kvh, into sl[g][row of the tile] (-inf on invalid rows).
template <typename T, int D>
__device__ __forceinline__ void dec_tile_logits(const DecArgs& a, int kvh, int G, int g0, int gn, const float (&kf)[kDecRpg][DecTile<T, D>::EPL],
                                                const bool (&valid)[kDecRpg], float (*sl)[DecTile<T, D>::ROWS]) {
    using TL = DecTile<T, D>;
    const int lane_in = threadIdx.x % TL::LPR, grp = threadIdx.x / TL::LPR;
    const T* q = reinterpret_cast<const T*>(a.q);
#pragma unroll
    for (int g = 0; g < kDecGmax; ++g) {
        if (g < gn) {
            float qf[TL::EPL];
            dec_unpack<T>(*reinterpret_cast<const uint4*>(q + (int64_t)(kvh * G + g0 + g) * a.q_sh + lane_in * TL::EPL), qf);
#pragma unroll
            for (int i = 0; i < kDecRpg; ++i) {
                float d = 0.f;
#pragma unroll
                for (int e = 0; e < TL::EPL; ++e) d = fmaf(qf[e], kf[i][e], d);
                d = dec_group_sum<TL::LPR>(d);
                if (lane_in == 0) sl[g][i * TL::GROUPS + grp] = valid[i] ? d * a.scale : -INFINITY;
            }
        }
    }
}

// Per head of the sweep (one wave each, round robin): max of the tile, sl <- exp(sl - max), sum.  `raw` (scores) gets the logits first.
template <int ROWS>
__device__ __forceinline__ void dec_tile_softmax(int gn, float (*sl)[ROWS], float* sm, float* ss, float* raw, int64_t raw_stride, int nrows) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int g = wave; g < gn; g += kDecThreads / 64) {
        float x[(ROWS + 63) / 64];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < (ROWS + 63) / 64; ++j) {
            const int r = j * 64 + lane;
            x[j] = r < ROWS ? sl[g][r] : -INFINITY;
            if (raw && r < nrows) raw[g * raw_stride + r] = x[j];
            m = fmaxf(m, x[j]);
        }
        m = dec_wave_max(m);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < (ROWS + 63) / 64; ++j) {
            const int r = j * 64 + lane;
            // an invalid row contributes nothing, also where the whole tile is invalid (m = -inf: not exp(-inf + inf)).  Keyed on the
            // row, not on m: fmaxf drops NaN, so a tile whose valid rows are all NaN has m = -inf too, and NaN - (-inf) stays NaN.
            const float p = x[j] == -INFINITY ? 0.f : expf(x[j] - m);
            if (r < ROWS) sl[g][r] = p;
            s += p;
        }
        s = wave_sum(s);
        if (lane == 0) { sm[g] = m; ss[g] = s; }
    }
}

template <typename T, int D>
__global__ void __launch_bounds__(kDecThreads) k_dec_logits(DecArgs a) {
    using TL = DecTile<T, D>;
    __shared__ float sl[kDecGmax][TL::ROWS];
    __shared__ float sm[kDecGmax], ss[kDecGmax];
    const int lane_in = threadIdx.x % TL::LPR, grp = threadIdx.x / TL::LPR;
    const int tile = blockIdx.x, kvh = blockIdx.y, G = a.Hq / a.Hkv;
    const int row0 = tile * TL::ROWS;
    const T* kb = reinterpret_cast<const T*>(a.k) + (int64_t)kvh * a.k_sh + lane_in * TL::EPL;
    float kf[kDecRpg][TL::EPL];
    bool valid[kDecRpg];
#pragma unroll
    for (int i = 0; i < kDecRpg; ++i) {
        const int r = row0 + i * TL::GROUPS + grp;
        valid[i] = r < a.Lk;
        uint4 u = make_uint4(0u, 0u, 0u, 0u);
        if (valid[i]) u = *reinterpret_cast<const uint4*>(kb + (int64_t)r * a.k_sl);
        dec_unpack<T>(u, kf[i]);
    }
    const int nrows = a.Lk - row0 < TL::ROWS ? a.Lk - row0 : TL::ROWS;
    for (int g0 = 0; g0 < G; g0 += kDecGmax) {
        const int gn = G - g0 < kDecGmax ? G - g0 : kDecGmax;
        dec_tile_logits<T, D>(a, kvh, G, g0, gn, kf, valid, sl);
        __syncthreads();
        dec_tile_softmax<TL::ROWS>(gn, sl, sm, ss, a.logits + (int64_t)(kvh * G + g0) * a.Lk + row0, a.Lk, nrows);
        __syncthreads();
        if ((int)threadIdx.x < gn) {
            float* p = a.part + ((int64_t)tile * a.Hq + kvh * G + g0 + threadIdx.x) * 2;
            p[0] = sm[threadIdx.x]; p[1] = ss[threadIdx.x];
        }
        __syncthreads();
    }
}

constexpr int kDecMaxHq = 256;

__global__ void __launch_bounds__(kDecThreads) k_dec_score(DecArgs a, int tiles, float* __restrict__ score) {
    __shared__ float sM[kDecMaxHq], sS[kDecMaxHq];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int h = wave; h < a.Hq; h += kDecThreads / 64) {
        float m = -INFINITY;
        for (int t = lane; t < tiles; t += 64) m = fmaxf(m, a.part[((int64_t)t * a.Hq + h) * 2]);
        m = dec_wave_max(m);
        float s = 0.f;
        for (int t = lane; t < tiles; t += 64) {
            const float* p = a.part + ((int64_t)t * a.Hq + h) * 2;
            s += p[1] * expf(p[0] - m);
        }
        s = wave_sum(s);
        if (lane == 0) { sM[h] = m; sS[h] = s; }
    }
    __syncthreads();
    const int j = blockIdx.x * kDecThreads + threadIdx.x;
    if (j >= a.Lk) return;
    float acc = 0.f;
    for (int h = 0; h < a.Hq; ++h) acc += expf(a.logits[(int64_t)h * a.Lk + j] - sM[h]) / sS[h];
    score[j] = acc / (float)a.Hq;
}

// ---- selection ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t dec_key(float x) { return x > 0.f ? __float_as_uint(x) : 0u; }

__global__ void __launch_bounds__(1024) k_dec_select(const float* __restrict__ score, int start, int window, int num_keep, int tail_from,
                                                     int tail_len, int32_t* __restrict__ keep) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_prefix, s_need;
    __shared__ uint32_t wtot[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < start; i += 1024) keep[i] = i;
    for (int i = tid; i < tail_len; i += 1024) keep[start + num_keep + i] = tail_from + i;
    if (num_keep == 0) return;
    const float* w = score + start;
    // the num_keep-th largest key of the window: theta; need = how many entries equal to theta are kept
    uint32_t prefix = 0u, mask = 0u, need = (uint32_t)num_keep;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        for (int i = tid; i < window; i += 1024) {
            const uint32_t key = dec_key(w[i]);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (wave == 0) {
            const uint32_t c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
            const uint32_t tot = c0 + c1 + c2 + c3;
            uint32_t suf = tot;                               // entries in the bins of this lane and of the lanes above
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t t = __shfl_down(suf, off, 64);
                if (lane + off < 64) suf += t;
            }
            const uint32_t above = suf - tot;
            if (above < need && need <= suf) {
                uint32_t rem = need - above, bin;
                if (c3 >= rem) bin = 3u;
                else if (c3 + c2 >= rem) { bin = 2u; rem -= c3; }
                else if (c3 + c2 + c1 >= rem) { bin = 1u; rem -= c3 + c2; }
                else { bin = 0u; rem -= c3 + c2 + c1; }
                s_prefix = prefix | ((4u * lane + bin) << shift);
                s_need = rem;
            }
        }
        __syncthreads();
        prefix = s_prefix;
        need = s_need;
        mask |= 255u << shift;
    }
    const uint32_t theta = prefix;
    // ordered compaction: entry i goes to (entries above theta before i) + min(entries equal to theta before i, need)
    uint32_t gt_base = 0u, eq_base = 0u;
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int base = 0; base < window; base += 1024) {
        const int i = base + tid;
        const uint32_t key = i < window ? dec_key(w[i]) : 0u;
        const bool gt = i < window && key > theta, eq = i < window && key == theta;
        const uint64_t bgt = __ballot(gt), beq = __ballot(eq);
        if (lane == 0) wtot[wave] = (uint32_t)__popcll(bgt) | ((uint32_t)__popcll(beq) << 16);
        __syncthreads();
        uint32_t pre_gt = 0u, pre_eq = 0u, tot_gt = 0u, tot_eq = 0u;
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const uint32_t t = wtot[x];
            tot_gt += t & 0xffffu; tot_eq += t >> 16;
            if (x < wave) { pre_gt += t & 0xffffu; pre_eq += t >> 16; }
        }
        const uint32_t g_before = gt_base + pre_gt + (uint32_t)__popcll(bgt & below);
        const uint32_t e_before = eq_base + pre_eq + (uint32_t)__popcll(beq & below);
        if (gt || (eq && e_before < need)) {
            const uint32_t pos = g_before + (e_before < need ? e_before : need);
            if (pos < (uint32_t)num_keep) keep[start + pos] = start + i;
        }
        gt_base += tot_gt; eq_base += tot_eq;
        __syncthreads();
    }
}

// ---- gathered attention ------------------------------------------------------------------------------------------------------
template <typename T, int D>
__global__ void __launch_bounds__(kDecThreads) k_dec_gathered(DecArgs a) {
    using TL = DecTile<T, D>;
    __shared__ float sl[kDecGmax][TL::ROWS];
    __shared__ float sm[kDecGmax], ss[kDecGmax];
    __shared__ float red[kDecThreads / 64][kDecGmax][D];
    const int lane_in = threadIdx.x % TL::LPR, grp = threadIdx.x / TL::LPR, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x, kvh = blockIdx.y, G = a.Hq / a.Hkv;
    const T* kb = reinterpret_cast<const T*>(a.k) + (int64_t)kvh * a.k_sh + lane_in * TL::EPL;
    const T* vb = reinterpret_cast<const T*>(a.v) + (int64_t)kvh * a.v_sh + lane_in * TL::EPL;
    bool valid[kDecRpg];
    int row[kDecRpg];
#pragma unroll
    for (int i = 0; i < kDecRpg; ++i) {
        const int e = tile * TL::ROWS + i * TL::GROUPS + grp;
        valid[i] = e < a.n_keep;
        row[i] = valid[i] ? a.keep[e] : 0;
        if (row[i] < 0 || row[i] >= a.Lk) { valid[i] = false; row[i] = 0; }     // never read outside the cache
    }
    uint4 ku[kDecRpg], vu[kDecRpg];
#pragma unroll
    for (int i = 0; i < kDecRpg; ++i) {
        ku[i] = make_uint4(0u, 0u, 0u, 0u);
        vu[i] = make_uint4(0u, 0u, 0u, 0u);
        if (valid[i]) {
            ku[i] = *reinterpret_cast<const uint4*>(kb + (int64_t)row[i] * a.k_sl);
            vu[i] = *reinterpret_cast<const uint4*>(vb + (int64_t)row[i] * a.v_sl);
        }
    }
    float kf[kDecRpg][TL::EPL];
#pragma unroll
    for (int i = 0; i < kDecRpg; ++i) dec_unpack<T>(ku[i], kf[i]);
    for (int g0 = 0; g0 < G; g0 += kDecGmax) {
        const int gn = G - g0 < kDecGmax ? G - g0 : kDecGmax;
        dec_tile_logits<T, D>(a, kvh, G, g0, gn, kf, valid, sl);
        __syncthreads();
        dec_tile_softmax<TL::ROWS>(gn, sl, sm, ss, nullptr, 0, 0);
        __syncthreads();
        float acc[kDecGmax][TL::EPL];
#pragma unroll
        for (int g = 0; g < kDecGmax; ++g)
#pragma unroll
            for (int e = 0; e < TL::EPL; ++e) acc[g][e] = 0.f;
#pragma unroll
        for (int i = 0; i < kDecRpg; ++i) {
            float vf[TL::EPL];
            dec_unpack<T>(vu[i], vf);
#pragma unroll
            for (int g = 0; g < kDecGmax; ++g) {
                if (g < gn) {
                    const float p = sl[g][i * TL::GROUPS + grp];
#pragma unroll
                    for (int e = 0; e < TL::EPL; ++e) acc[g][e] = fmaf(p, vf[e], acc[g][e]);
                }
            }
        }
        // the lane groups of a wave (same lane_in), then the four waves through LDS
#pragma unroll
        for (int g = 0; g < kDecGmax; ++g) {
            if (g < gn) {
#pragma unroll
                for (int e = 0; e < TL::EPL; ++e) {
                    float x = acc[g][e];
#pragma unroll
                    for (int off = TL::LPR; off < 64; off <<= 1) x += __shfl_xor(x, off, 64);
                    acc[g][e] = x;
                }
                if ((threadIdx.x & 63) < TL::LPR) {
#pragma unroll
                    for (int e = 0; e < TL::EPL; ++e) red[wave][g][lane_in * TL::EPL + e] = acc[g][e];
                }
            }
        }
        __syncthreads();
        for (int x = threadIdx.x; x < gn * D; x += kDecThreads) {
            const int g = x / D, d = x - g * D;
            const float s = (red[0][g][d] + red[1][g][d]) + (red[2][g][d] + red[3][g][d]);
            a.pacc[((int64_t)tile * a.Hq + kvh * G + g0 + g) * D + d] = s;
        }
        if ((int)threadIdx.x < gn) {
            float* p = a.part + ((int64_t)tile * a.Hq + kvh * G + g0 + threadIdx.x) * 2;
            p[0] = sm[threadIdx.x]; p[1] = ss[threadIdx.x];
        }
        __syncthreads();
    }
}

template <typename T> __device__ __forceinline__ void dec_store(T* p, float f);
template <> __device__ __forceinline__ void dec_store<float>(float* p, float f) { *p = f; }
template <> __device__ __forceinline__ void dec_store<bf16_t>(bf16_t* p, float f) { p->x = (uint16_t)float_to_bf16_bits(f); }
template <> __device__ __forceinline__ void dec_store<f16_t>(f16_t* p, float f) { p->x = (uint16_t)float_to_f16_bits(f); }

template <typename T, int D>
__global__ void __launch_bounds__(kDecThreads) k_dec_combine(DecArgs a, int tiles, T* __restrict__ out) {
    constexpr int SUB = kDecThreads / D;
    __shared__ float smax[kDecThreads / 64];
    __shared__ float racc[SUB][D], rsum[SUB];
    const int h = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int d = threadIdx.x % D, sub = threadIdx.x / D;
    float m = -INFINITY;
    for (int t = threadIdx.x; t < tiles; t += kDecThreads) m = fmaxf(m, a.part[((int64_t)t * a.Hq + h) * 2]);
    m = dec_wave_max(m);
    if (lane == 0) smax[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    float s = 0.f, o = 0.f;
    for (int t = sub; t < tiles; t += SUB) {
        const float* p = a.part + ((int64_t)t * a.Hq + h) * 2;
        const float wgt = expf(p[0] - m);
        s = fmaf(wgt, p[1], s);
        o = fmaf(wgt, a.pacc[((int64_t)t * a.Hq + h) * D + d], o);
    }
    racc[sub][d] = o;
    if (d == 0) rsum[sub] = s;
    __syncthreads();
    if (sub == 0) {
        float so = 0.f, sw = 0.f;
#pragma unroll
        for (int x = 0; x < SUB; ++x) { so += racc[x][d]; sw += rsum[x]; }
        dec_store<T>(out + (int64_t)h * D + d, so / sw);
    }
}

template <typename F> hipError_t dec_dispatch(int dtype, int D, F f) {
    if (dtype == STTM_F32) return D == 64 ? f(float{}, std::integral_constant<int, 64>{}) : f(float{}, std::integral_constant<int, 128>{});
    if (dtype == STTM_BF16) return D == 64 ? f(bf16_t{}, std::integral_constant<int, 64>{}) : f(bf16_t{}, std::integral_constant<int, 128>{});
    return D == 64 ? f(f16_t{}, std::integral_constant<int, 64>{}) : f(f16_t{}, std::integral_constant<int, 128>{});
}

int decode_tile_rows(int dtype, int D) { return kDecRpg * kDecThreads / (D * (dtype == STTM_F32 ? 4 : 2) / 16); }

hipError_t launch_decode_scores(const void* q, int64_t q_sh, const void* k, int64_t k_sh, int64_t k_sl, int Hq, int Hkv, int Lk, int D,
                                int dtype, float scale, float* logits, float* part, float* score, hipStream_t stream) {
    DecArgs a = {};
    a.q = q; a.q_sh = q_sh; a.k = k; a.k_sh = k_sh; a.k_sl = k_sl; a.Hq = Hq; a.Hkv = Hkv; a.Lk = Lk; a.scale = scale;
    a.logits = logits; a.part = part;
    const int rows = decode_tile_rows(dtype, D);
    const int tiles = (Lk + rows - 1) / rows;
    (void)dec_dispatch(dtype, D, [&](auto t, auto d) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_dec_logits<T, decltype(d)::value>), dim3(tiles, Hkv), dim3(kDecThreads), 0, stream, a);
        return hipSuccess;
    });
    hipLaunchKernelGGL(k_dec_score, dim3((Lk + kDecThreads - 1) / kDecThreads), dim3(kDecThreads), 0, stream, a, tiles, score);
    return hipGetLastError();
}

hipError_t launch_decode_select(const float* score, int start, int window, int num_keep, int tail_from, int tail_len, int32_t* keep,
                                hipStream_t stream) {
    hipLaunchKernelGGL(k_dec_select, dim3(1), dim3(1024), 0, stream, score, start, window, num_keep, tail_from, tail_len, keep);
    return hipGetLastError();
}

hipError_t launch_decode_gathered(const void* q, int64_t q_sh, const void* k, int64_t k_sh, int64_t k_sl, const void* v, int64_t v_sh,
                                  int64_t v_sl, int Hq, int Hkv, int Lk, int D, int dtype, float scale, const int32_t* keep, int n_keep,
                                  float* part, float* pacc, void* out, hipStream_t stream) {
    DecArgs a = {};
    a.q = q; a.q_sh = q_sh; a.k = k; a.k_sh = k_sh; a.k_sl = k_sl; a.v = v; a.v_sh = v_sh; a.v_sl = v_sl;
    a.Hq = Hq; a.Hkv = Hkv; a.Lk = Lk; a.scale = scale; a.keep = keep; a.n_keep = n_keep; a.part = part; a.pacc = pacc;
    const int rows = decode_tile_rows(dtype, D);
    const int tiles = (n_keep + rows - 1) / rows;
    (void)dec_dispatch(dtype, D, [&](auto t, auto d) {
        using T = decltype(t);
        constexpr int DD = decltype(d)::value;
        hipLaunchKernelGGL((k_dec_gathered<T, DD>), dim3(tiles, Hkv), dim3(kDecThreads), 0, stream, a);
        hipLaunchKernelGGL((k_dec_combine<T, DD>), dim3(Hq), dim3(kDecThreads), 0, stream, a, tiles, reinterpret_cast<T*>(out));
        return hipSuccess;
    });
    return hipGetLastError();
}

}  // namespace sttm
