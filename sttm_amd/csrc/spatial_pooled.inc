// K1 reading the UNPOOLED token map: get_2dPool fused into the spatial kernel's leaf load (SURVEY 8f rank 2, round 5).
//
// The frame descriptor points at the unpooled map ([src_h, src_w, C] rows, e.g. the 27 x 27 SigLIP grid behind the projector) and
// leaf (y, x) of the quadtree's H x W grid is built from its four source tokens exactly as LlavaMetaForCausalLM.get_2dPool builds it
// (llava/model/llava_arch.py:173-198 of the reference): bilinear F.interpolate(size = ceil(side / stride)), or a 2 x 2 average / max
// window -- float32 arithmetic with one rounding per operation in the order of csrc/pool2d.hip (= oracle/pool_oracle.py = ATen), then
// ONE rounding to the input dtype, which is what the stand-alone pooling kernel writes and the spatial stage would read back.  The
// pooled map is never written or re-read.
//
// Round-5 measurements behind the shape of this file: one memory round trip per leaf ran the bf16 C = 3584 stage at 3.6 TB/s; the
// taps computed per thread (two fused multiply-adds, conversions and clamps per axis and leaf, all uniform) and element-wise 16-bit
// unpack / insert made the stage VALU-bound.  Now the taps are a kernel-argument table (scalar loads), the arithmetic runs on channel
// PAIRS (v_pk_mul_f32 / v_pk_add_f32, one v_cvt_pk per pair), and two leaves (eight source rows) are requested per round trip.
#pragma once
#include "quadtree_spatial.inc"

#ifndef STTM_POOLED_PER_16
#define STTM_POOLED_PER_16 2          // leaves of 16-bit packs per memory round trip (1: half the source rows in flight)
#endif

namespace sttm {

typedef float pool_f2 __attribute__((ext_vector_type(2)));

template <typename T, int VEC>
__device__ __forceinline__ pool_f2 pack_pair(const Pack<T, VEC>& p, int i) {          // channels i, i + 1 (i even) as floats
    if constexpr (TypeInfo<T>::bytes == 4) {
        return pool_f2{p.v[i], p.v[i + 1]};
    } else if constexpr (std::is_same<T, bf16_t>::value) {
        const uint32_t w = p.w[i >> 1];
        return pool_f2{__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)};
    } else {
        const sttm_cvt_f16x2 h = __builtin_bit_cast(sttm_cvt_f16x2, p.w[i >> 1]);
        return __builtin_convertvector(h, pool_f2);
    }
}

struct PoolTaps { uint32_t o00, o01, o10, o11; float h0, h1, w0, w1; };
__device__ __forceinline__ PoolTaps pool_taps(const SpatialCtx& cx, int y, int x) {
    const PoolTable& tb = *cx.ptab;
    PoolTaps t;
    const uint32_t r0 = (uint32_t)tb.i0[0][y] * cx.sHb, r1 = (uint32_t)tb.i1[0][y] * cx.sHb;
    const uint32_t c0 = (uint32_t)tb.i0[1][x] * cx.sWb, c1 = (uint32_t)tb.i1[1][x] * cx.sWb;
    t.o00 = r0 + c0; t.o01 = r0 + c1; t.o10 = r1 + c0; t.o11 = r1 + c1;
    t.h0 = tb.l0[0][y]; t.h1 = tb.l1[0][y]; t.w0 = tb.l0[1][x]; t.w1 = tb.l1[1][x];
    return t;
}

template <typename T, int VEC>
__device__ __forceinline__ Pack<T, VEC> pool_combine(int mode, const PoolTaps& t, const Pack<T, VEC>& p00, const Pack<T, VEC>& p01,
                                                     const Pack<T, VEC>& p10, const Pack<T, VEC>& p11) {
#pragma clang fp contract(off)
    static_assert(VEC % 2 == 0, "the pooled leaf load works on channel pairs");
    Pack<T, VEC> res;
#pragma unroll
    for (int e = 0; e < VEC; e += 2) {
        const pool_f2 a = pack_pair<T, VEC>(p00, e), b = pack_pair<T, VEC>(p01, e), c = pack_pair<T, VEC>(p10, e), d = pack_pair<T, VEC>(p11, e);
        pool_f2 r;
        if (mode == STTM_POOL_BILINEAR) {                      // (uniform)
            const pool_f2 top = t.w0 * a + t.w1 * b;
            const pool_f2 bot = t.w0 * c + t.w1 * d;
            r = t.h0 * top + t.h1 * bot;
        } else if (mode == STTM_POOL_MAX) {
            // k_pool2d's (= ATen's) rule: (val > maxval) || isnan(val), so a NaN in the window reaches the leaf
            pool_f2 m = {-INFINITY, -INFINITY};
            m.x = (a.x > m.x || a.x != a.x) ? a.x : m.x; m.y = (a.y > m.y || a.y != a.y) ? a.y : m.y;
            m.x = (b.x > m.x || b.x != b.x) ? b.x : m.x; m.y = (b.y > m.y || b.y != b.y) ? b.y : m.y;
            m.x = (c.x > m.x || c.x != c.x) ? c.x : m.x; m.y = (c.y > m.y || c.y != c.y) ? c.y : m.y;
            m.x = (d.x > m.x || d.x != d.x) ? d.x : m.x; m.y = (d.y > m.y || d.y != d.y) ? d.y : m.y;
            r = m;
        } else {
            const pool_f2 z = {0.f, 0.f};
            r = ((((z + a) + b) + c) + d) / 4.f;
        }
        res.set_pair(e, r.x, r.y);
    }
    return res;
}

// the four leaves of one mid, two per memory round trip (eight source rows in flight per lane; all sixteen rows of a mid at once spill
// next to the twelve leaves already built)
template <typename T, int VEC>
__device__ __forceinline__ void load_quad_pooled(const SpatialCtx& cx, const int (&y)[4], const int (&x)[4], const bool (&valid)[4],
                                                 Pack<T, VEC> (&leaf)[4]) {
    // PER = leaves per memory round trip: two for fp32 packs (eight source rows in flight), STTM_POOLED_PER_16 for 16-bit packs
    constexpr int PER = TypeInfo<T>::lowp ? STTM_POOLED_PER_16 : 2;
#pragma unroll
    for (int h = 0; h < 4 / PER; ++h) {
        PoolTaps t[PER];
        Pack<T, VEC> p[PER][4];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int q = PER * h + j;
            t[j] = pool_taps(cx, valid[q] ? y[q] : 0, valid[q] ? x[q] : 0);
            p[j][0] = load_leaf_at<T, VEC>(cx, t[j].o00, valid[q]);
            p[j][1] = load_leaf_at<T, VEC>(cx, t[j].o01, valid[q]);
            p[j][2] = load_leaf_at<T, VEC>(cx, t[j].o10, valid[q]);
            p[j][3] = load_leaf_at<T, VEC>(cx, t[j].o11, valid[q]);
        }
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int q = PER * h + j;
            if (valid[q]) leaf[q] = pool_combine<T, VEC>(cx.pool_mode, t[j], p[j][0], p[j][1], p[j][2], p[j][3]);
            else leaf[q].zero();
        }
    }
}

// The spatial stage of a 3-level tree on the unpooled map: same body, same outputs as k_spatial on the pooled map; 16-byte packs,
// whole-vector cosine.  Every emitted node -- also the 1 x 1 ones -- goes to the scratch matrix S (leaves_in_x = 0: the pooled tokens
// exist nowhere else).
template <typename T, int VEC, int MAXNT>
__global__ void __launch_bounds__(MAXNT, 4) k_spatial_pooled(const SpatialArgs a0, const BatchPtrs bp, const PoolTable tab) {
    SpatialArgs a = a0;
    rebase(a, bp, blockIdx.y);
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* part = reinterpret_cast<float*>(smem_raw);             // [nwave][NSTAT]
    const int nwave = blockDim.x / kWave;
    const LevelDims& g = a.dims;
    const int R = g.h[0] * g.w[0];
    // all root cells of one frame on one XCD (k_spatial's mapping): here the alias leaves cost FOUR source rows each
    const int xcd_slot = blockIdx.x & 7, per_xcd = blockIdx.x >> 3;
    const int t = (per_xcd / R) * 8 + xcd_slot, rcell = per_xcd % R;
    if (t >= a.T) return;
    const int I = rcell / g.w[0], J = rcell % g.w[0];
    SpatialCtx cx;
    spatial_ctx_init<T>(cx, a, t, threadIdx.x, VEC);
    cx.ptab = &tab;
    const bool interior = !(I == 0 && ((g.h[1] | g.h[2]) & 1)) && !(J == 0 && ((g.w[1] | g.w[2]) & 1));
    if (interior) spatial_block3<T, VEC, true, false, true>(a, cx, t, I, J, t * R + rcell, part, nwave);
    else spatial_block3<T, VEC, false, false, true>(a, cx, t, I, J, t * R + rcell, part, nwave);
}

// the taps of one axis, with the device's own arithmetic (bilinear_tap of sttm_common.h: one fused multiply-add, one rounding per operation)
inline void pool_axis_table(int mode, int n_in, int n_out, float scale, int* i0, int* i1, float* l0, float* l1) {
    for (int o = 0; o < kPoolMaxSide; ++o) {
        if (o >= n_out) { i0[o] = i1[o] = 0; l0[o] = l1[o] = 0.f; continue; }
        if (mode == STTM_POOL_BILINEAR) {
            float src = __builtin_fmaf(scale, (float)o + 0.5f, -0.5f);
            src = src < 0.f ? 0.f : src;
            i0[o] = (int)src;
            i1[o] = i0[o] + 1 < n_in ? i0[o] + 1 : n_in - 1;
            l1[o] = src - (float)i0[o];
            l0[o] = 1.f - l1[o];
        } else {
            i0[o] = 2 * o; i1[o] = 2 * o + 1; l0[o] = l1[o] = 0.f;
        }
    }
}

template <typename T>
hipError_t launch_spatial_pooled_t(const SpatialArgs& a, const BatchPtrs& bp, int n_videos, int nt, hipStream_t stream) {
    constexpr int VEC = 16 / (int)TypeInfo<T>::bytes;
    if (a.H > kPoolMaxSide || a.W > kPoolMaxSide) return hipErrorInvalidValue;
    PoolTable tab;
    pool_axis_table(a.pool_mode, a.src_h, a.H, a.pool_sh, tab.i0[0], tab.i1[0], tab.l0[0], tab.l1[0]);
    pool_axis_table(a.pool_mode, a.src_w, a.W, a.pool_sw, tab.i0[1], tab.i1[1], tab.l0[1], tab.l1[1]);
    const int grid = (a.T + 7) / 8 * 8 * a.dims.h[0] * a.dims.w[0];
    const size_t smem = sizeof(float) * (size_t)(nt / kWave) * TreeConst<3>::NSTAT;
    const dim3 g3(grid, n_videos);
    if (nt <= 256) hipLaunchKernelGGL((k_spatial_pooled<T, VEC, 256>), g3, dim3(nt), smem, stream, a, bp, tab);
    else if (nt <= 512) hipLaunchKernelGGL((k_spatial_pooled<T, VEC, 512>), g3, dim3(nt), smem, stream, a, bp, tab);
    else hipLaunchKernelGGL((k_spatial_pooled<T, VEC, 1024>), g3, dim3(nt), smem, stream, a, bp, tab);
    return hipGetLastError();
}

}  // namespace sttm
