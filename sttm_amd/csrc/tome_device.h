// Small device helpers shared by the ToMe translation units (tome.hip: one clip per call; tome_snippet.hip: many short segments per
// call): the packed score / rank keys, the rounding of 16-bit intermediates, typed element access, the MFMA wrappers, the fp16
// two-plane split constants and the per-lane running max of a transposed score tile.  Kernels stay in their own files.
#pragma once
#include "sttm_kernels.h"

namespace sttm {

__device__ __forceinline__ unsigned long long pack_score(float v, int j) {
    // order-preserving map of the float, then "smaller j wins" on ties (torch.max returns the first maximum)
    unsigned u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned long long)(0xffffffffu - (unsigned)j);
}

// Running max / argmax of one lane's scores of a 64 (j) x 32*QI (i) wave tile: acc[p][q][e] is the score of a-row q against
// candidate  jlane + p*32 + (e&3) + 8*(e>>2)  (jlane = tile origin + wave's j offset + 4 * lane half).  A lane meets its candidates in
// ascending j -- inside a tile and from tile to tile -- so the first maximum (torch.max; tome_token_merger.py:36) is the first score
// STRICTLY above the running one: for tiles that lie inside [0, nb) that is a compare and two selects per score, no branch.
// Only the last, partial tile takes the general form (round 2's, which cost ~30 instructions and an exec-mask branch per score).
typedef float tome_f32x16 __attribute__((ext_vector_type(16)));
template <int QI, typename RoundFn, int PJ = 2>
__device__ __forceinline__ void tome_running_max(const tome_f32x16 (&acc)[PJ][QI], float (&bestv)[QI], int (&bestj)[QI], int jlane, int nb,
                                                 bool inside, RoundFn rnd) {
    static_assert(PJ != 4, "the four-wave kernel has its own running max (tome_running_max_agpr)");
    if (inside) {
#pragma unroll
        for (int q = 0; q < QI; ++q) {
            float bv = bestv[q];
            int bc = -1;
#pragma unroll
            for (int p = 0; p < PJ; ++p) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float v = rnd(acc[p][q][e]);
                    const bool gt = v > bv;
                    bc = gt ? p * 32 + (e & 3) + 8 * (e >> 2) : bc;
                    bv = gt ? v : bv;
                }
            }
            bestj[q] = bc >= 0 ? jlane + bc : bestj[q];
            bestv[q] = bv;
        }
    } else {
#pragma unroll
        for (int q = 0; q < QI; ++q)
#pragma unroll
            for (int p = 0; p < PJ; ++p)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int j = jlane + p * 32 + (e & 3) + 8 * (e >> 2);
                    const float v = rnd(acc[p][q][e]);
                    if (j < nb && (v > bestv[q] || (v == bestv[q] && j < bestj[q]))) { bestv[q] = v; bestj[q] = j; }
                }
    }
}

// ---------------------------------------------------------------------------------------------------
// 16-bit inputs (bfloat16 / float16): the reference runs the same torch ops on the hidden states' dtype
// (tome_attn_monkey_patch.py:88-107 with a bf16 model), so every intermediate tensor is ROUNDED to that dtype:
// the unit rows, the scores (an fp32-accumulating matmul whose result is stored in 16 bits -- hence many exact ties,
// first maximum = smaller j), x * size, every scatter-add step, the final division.  Matrix products run on
// v_mfma_f32_32x32x16_{bf16,f16} (16x the fp32-input rate).
// ---------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ float tome_round(float f);
template <> __device__ __forceinline__ float tome_round<float>(float f) { return f; }
template <> __device__ __forceinline__ float tome_round<bf16_t>(float f) { return bf16_bits_to_float(float_to_bf16_bits(f)); }
template <> __device__ __forceinline__ float tome_round<f16_t>(float f) { return f16_bits_to_float(float_to_f16_bits(f)); }
template <typename T> __device__ __forceinline__ float tome_ld(const void* p, int64_t i);
template <> __device__ __forceinline__ float tome_ld<float>(const void* p, int64_t i) { return reinterpret_cast<const float*>(p)[i]; }
template <> __device__ __forceinline__ float tome_ld<bf16_t>(const void* p, int64_t i) { return bf16_bits_to_float(reinterpret_cast<const uint16_t*>(p)[i]); }
template <> __device__ __forceinline__ float tome_ld<f16_t>(const void* p, int64_t i) { return f16_bits_to_float(reinterpret_cast<const uint16_t*>(p)[i]); }
template <typename T> __device__ __forceinline__ void tome_st(void* p, int64_t i, float v);
template <> __device__ __forceinline__ void tome_st<float>(void* p, int64_t i, float v) { reinterpret_cast<float*>(p)[i] = v; }
template <> __device__ __forceinline__ void tome_st<bf16_t>(void* p, int64_t i, float v) { reinterpret_cast<uint16_t*>(p)[i] = (uint16_t)float_to_bf16_bits(v); }
template <> __device__ __forceinline__ void tome_st<f16_t>(void* p, int64_t i, float v) { reinterpret_cast<uint16_t*>(p)[i] = (uint16_t)float_to_f16_bits(v); }

typedef __bf16 tome_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 tome_f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef unsigned int tome_u32x4 __attribute__((ext_vector_type(4)));      // 16-byte staging unit (a native vector: stays in registers)
template <typename T> struct TomeMfma;
template <> struct TomeMfma<bf16_t> {
    typedef tome_bf16x8 vec;
    static __device__ __forceinline__ f32x16_t run(vec a, vec b, f32x16_t c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct TomeMfma<f16_t> {
    typedef tome_f16x8 vec;
    static __device__ __forceinline__ f32x16_t run(vec a, vec b, f32x16_t c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

// fp32 inputs on the 16-bit matrix pipe: every unit-row element v is written as 4096 * v = h + l + e with two fp16 planes h, l
// (the error analysis is in front of k_tome_normalize_split, tome.hip)
constexpr float kSplitScale = 4096.f;
constexpr float kSplitUnscale = 1.f / (4096.f * 4096.f);

// rank key of a-token i from its packed best score: descending score, ties to the smaller index; all keys are distinct
__device__ __forceinline__ unsigned long long tome_rank_key(unsigned long long b, int i) {
    const unsigned ku = b ? (unsigned)(b >> 32) : 0xffc00000u;          // no finite score at all: a NaN row (sorts first)
    return ((unsigned long long)ku << 32) | (unsigned long long)(0xffffffffu - (unsigned)i);
}

// Poisoned b-rows.  The reference divides by the norm without an eps, so a token with a NaN, an Inf (inf / inf) or nothing but zeros
// (0 / 0) has a unit row that holds a NaN, and a token whose sum of squares underflows (norm 0) has a unit row of +-Inf.  EVERY score
// against such a row is NaN -- NaN products, or infinities of both signs in one sum -- and torch.max propagates NaN and returns the
// first NaN's index: with such a b-row j* every a-row's (node_max, node_idx) is (NaN, j*) -- (NaN, 0) for an a-row that is poisoned
// itself, whose scores are all NaN.  The running maxima of the match kernels skip NaN scores (a compare with NaN is false), which is
// right for the poisoned a-row (no score wins: its packed best stays 0 = a NaN row with index 0) and wrong for a clean a-row facing j*.
// The match kernels stay as they are: the normalise kernels, which visit every unit row anyway, note the smallest b-row with a
// non-finite unit row (`poison` word: 0xffffffff - j* by atomicMax, 0 = none; per segment a flag per b-row in tome_snippet.hip), and
// the ranking kernels replace every row's packed best by (NaN, j*) when there is one.  A unit row can be non-finite only if the norm is
// 0, Inf or NaN -- one wave-uniform compare per row on clean inputs; only then are the row's elements looked at.
// (The one case this leaves to chance: against a +-Inf unit row of k elements an a-row whose k products all have one sign scores +-Inf
// in the reference, not NaN -- 2^-(k-1) of the a-rows, k = the metric width)
__device__ __forceinline__ bool tome_norm_degenerate(float nrm) { return !(nrm > 0.f && nrm < INFINITY); }
// with a degenerate norm: is elem / nrm non-finite?  norm 0 or NaN: always (+-Inf, 0 / 0 or NaN); norm Inf: iff elem is +-Inf or NaN.
// (Also right for an element that is already divided: then it is 0 or NaN under an Inf norm.)
__device__ __forceinline__ bool tome_unit_nonfinite(float elem, float nrm) { return !(nrm == INFINITY) || !(fabsf(elem) < INFINITY); }
__device__ __forceinline__ unsigned long long tome_poisoned_best(unsigned long long b, unsigned pw) {
    // pw = 0xffffffff - j*, which is pack_score's low word of candidate j*; 0xffc00000 = pack_score's high word of the quiet NaN.
    // b == 0 (no score of the row compared true: all NaN) keeps index 0, the first NaN of such a row.
    return (pw != 0u && b != 0ull) ? ((0xffc00000ull << 32) | (unsigned long long)pw) : b;
}

template <typename T, int VEC> __device__ __forceinline__ void tome_ld_vec(const void* x, int64_t off, float (&v)[VEC]) {
    if constexpr (VEC == 1) {
        v[0] = tome_ld<T>(x, off);
    } else {
        const Pack<T, VEC> p = load_pack<T, VEC>(x, off);
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = p.get(e);
    }
}
template <typename T, int VEC> __device__ __forceinline__ void tome_st_vec(void* x, int64_t off, const float (&v)[VEC]) {
    if constexpr (VEC == 1) {
        tome_st<T>(x, off, v[0]);
    } else {
        Pack<T, VEC> p;
        pack_fill<T, VEC>(p, [&](int e) { return v[e]; });
        store_pack<T, VEC>(x, off, p);
    }
}

}  // namespace sttm
