// K1 -- fused quadtree spatial stage for gfx950.
//
// One workgroup owns one (frame t, root cell) pair and does, without leaving the CU:
//   pyramid of the root cell (quadtree_spatial_merger.py:9-86 of the reference), all parent<->child cosine
//   statistics (quadtree_builder.py:41-66), the top-down split decision (:68-74) and the emission of the
//   surviving nodes (:26-37, :73-74).
//
// Mapping to the hardware
//   * thread <-> VEC consecutive channels; a token row is read with one 16-byte (fp32 x4 / bf16 x8)
//     coalesced load per lane, every leaf token of the root cell is read from HBM exactly once;
//   * the whole root-cell pyramid (16 leaves + 4 mids + 1 top for a 3-level tree) lives in VGPRs in the
//     input dtype, so emitted features are stored straight from registers (no LDS staging, no re-read);
//   * the 41 partial dot products / norms per 3-level block are reduced across the wave with a
//     butterfly transpose-reduce (~44 shuffles), then across waves through LDS in a fixed order, so the
//     decisions are deterministic run to run;
//   * decisions are taken by the first few threads from the reduced statistics in LDS.
//
// Node features are written to the scratch matrix S at row  t*H*W + y1*W + x1  (the node's origin leaf), so
// "sorted by (t, y1, x1)" (quadtree_builder.py:198-203) is simply ascending row order: no sort is needed.
#pragma once
#include "sttm_kernels.h"

#ifndef STTM_F32_SWAP
#define STTM_F32_SWAP 0          // (3 = in-place lane swaps: 0 bytes of scratch, measured neutral on the headline -- 28.85 vs 28.99 us -- so the
                                 //  fp32 kernel keeps the plain form; the statistics phase is hidden behind other workgroups' memory waits)
#endif

namespace sttm {

// lane-swap stages of the statistics butterfly (sttm_common.h: wave_reduce_many)
template <typename T> constexpr int kSwapStages = TypeInfo<T>::lowp ? 2 : STTM_F32_SWAP;

template <int D> struct TreeConst {
    static constexpr int NNODE = depth_base(D);          // nodes of a complete 4-ary tree with D levels
    static constexpr int NPAR = depth_base(D - 1);       // non-leaf nodes
    static constexpr int NLEAF = pow4(D - 1);
    static constexpr int NSTAT = NNODE + 4 * NPAR + D;   // norm2[node] | dot[parent][slot] | alias_norm2[level]
    __host__ __device__ static constexpr int dot_id(int parent, int k) { return NNODE + parent * 4 + k; }
    __host__ __device__ static constexpr int alias_id(int level) { return NNODE + 4 * NPAR + level; }
};

struct CellGeo {           // children of one cell: first child row/col and how many (1 or 2) per axis
    int rs, rc, cs, cc;
};
__device__ __forceinline__ CellGeo cell_children(const LevelDims& g, int lvl, int i, int j) {
    CellGeo c;
    c.rs = child_start(i, g.h[lvl + 1]);
    c.rc = child_count(i, g.h[lvl + 1]);
    c.cs = child_start(j, g.w[lvl + 1]);
    c.cc = child_count(j, g.w[lvl + 1]);
    return c;
}

// pool 4 child packs in slot order ((c0+c1)+c2)+c3 over the valid ones; avg divides by the child count.
template <typename T, int VEC>
__device__ __forceinline__ Pack<T, VEC> pool4(const Pack<T, VEC> (&c)[4], const bool (&v)[4], bool sum_mode) {
    Pack<T, VEC> out;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt += v[k] ? 1 : 0;
    const float scale = sum_mode ? 1.f : (cnt == 4 ? 0.25f : (cnt == 2 ? 0.5f : 1.f));
    // The validity flags are the same for every lane (geometry of the workgroup's root cell): ONE scalar branch per pooled node
    // picks the straight-line sum of its shape.  Written as per-element `if (v[k]) s += ...` every add came with a v_cndmask
    // (3 per channel and pooled node: 240 of the 3000 vector instructions of the 16-wide bf16 kernel, which is VALU-bound).
    // (Only for the 32-byte packs: in the 128-register kernels the four code shapes cost registers and the fp32 headline
    // kernel began to spill.)
    if constexpr (TypeInfo<T>::bytes * VEC < 32) {
        pack_fill(out, [&](int e) {
            float s = c[0].get(e);
            if (v[1]) s += c[1].get(e);
            if (v[2]) s += c[2].get(e);
            if (v[3]) s += c[3].get(e);
            return s * scale;
        });
    } else if (v[1] && v[2] && v[3]) {
        pack_fill(out, [&](int e) { return (((c[0].get(e) + c[1].get(e)) + c[2].get(e)) + c[3].get(e)) * scale; });
    } else if (v[1]) {                                   // one row of two (slot 0 is always valid for a valid parent)
        pack_fill(out, [&](int e) { return (c[0].get(e) + c[1].get(e)) * scale; });
    } else if (v[2]) {                                   // one column of two
        pack_fill(out, [&](int e) { return (c[0].get(e) + c[2].get(e)) * scale; });
    } else {
        pack_fill(out, [&](int e) { return c[0].get(e) * scale; });
    }
    return out;
}

// A 3-level block (top, 4 mids, 16 leaves) held in registers; BL == 2 uses top + mid[] as its leaves,
// BL == 1 only `top`.
template <typename T, int VEC> struct BlockRegs {
    Pack<T, VEC> leaf[4][4];
    Pack<T, VEC> mid[4];
    Pack<T, VEC> top;
};
struct BlockGeo {
    bool v1[4];
    bool v2[4][4];
    int ci[4], cj[4];          // level+1 coordinates of the 4 children
    int li[4][4], lj[4][4];    // level+2 coordinates of the 16 grandchildren
};

template <int BL>
__device__ __forceinline__ void block_geometry(const LevelDims& g, int lvl, int i, int j, bool valid, BlockGeo& b) {
    if constexpr (BL == 1) return;
    const CellGeo c = cell_children(g, lvl, i, j);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int dy = k >> 1, dx = k & 1;
        b.v1[k] = valid && dy < c.rc && dx < c.cc;
        b.ci[k] = c.rs + dy;
        b.cj[k] = c.cs + dx;
        if constexpr (BL == 3) {
            CellGeo m = cell_children(g, lvl + 1, b.v1[k] ? b.ci[k] : 0, b.v1[k] ? b.cj[k] : 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ey = q >> 1, ex = q & 1;
                b.v2[k][q] = b.v1[k] && ey < m.rc && ex < m.cc;
                b.li[k][q] = m.rs + ey;
                b.lj[k][q] = m.cs + ex;
            }
        }
    }
}

// Token rows are read with BUFFER loads: the descriptor points at the workgroup's frame, the row of leaf (y, x) is a SCALAR
// byte offset (two 32-bit scalar multiplies) and every lane adds ONE offset for its channels, the same for all leaves.  With
// flat loads every lane built the 64-bit address t*sT + y*sH + x*sW + c0 itself: three 64-bit multiply-adds and ~35
// instructions per leaf, ~1.5 us for the 16 leaves of a root cell before the last load was even issued.  (The host checks that a
// frame spans < 2 GiB and that the strides are not negative.)
struct SpatialCtx {
    __amdgpu_buffer_rsrc_t frame;   // this workgroup's frame of x
    uint32_t sHb, sWb;    // row / column strides in bytes
    uint32_t voff;        // byte offset of this thread's channels inside a token row (0 for inactive lanes)
    int64_t c0;           // first channel of this thread
    bool active;          // c0 < C
    bool sum_mode;
    const PoolTable* ptab;   // k_spatial_pooled: the source taps of every pooled row / column (a kernel argument), else unused
    int pool_mode;
};
template <typename T>
__device__ __forceinline__ void spatial_ctx_init(SpatialCtx& cx, const SpatialArgs& a, int t, int tid, int vec) {
    const char* fb = reinterpret_cast<const char*>(a.x) + (int64_t)t * a.sT * TypeInfo<T>::bytes;
    cx.frame = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(fb), 0, -1, 0x00020000);
    cx.sHb = (uint32_t)(a.sH * TypeInfo<T>::bytes);
    cx.sWb = (uint32_t)(a.sW * TypeInfo<T>::bytes);
    cx.c0 = (int64_t)tid * vec;
    cx.active = cx.c0 < a.C;
    cx.voff = cx.active ? (uint32_t)(cx.c0 * TypeInfo<T>::bytes) : 0u;
    cx.sum_mode = a.sum_mode != 0;
    cx.ptab = nullptr;
    cx.pool_mode = a.pool_mode;
}

typedef unsigned int sp_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int sp_u32x2 __attribute__((ext_vector_type(2)));

// (t is the workgroup's own frame: the descriptor already points at it).  Idle lanes (c0 >= C) are masked out of the load
// itself: zeroing their registers AFTER the load would make their wave wait for every single load (vmcnt(0) per leaf --
// measured: bf16 C = 3584 with 224 of 256 lanes busy, 66.6 -> 88 us).
template <typename T, int VEC>
__device__ __forceinline__ Pack<T, VEC> load_leaf(const SpatialCtx& cx, int /*t*/, int y, int x, bool valid) {
    Pack<T, VEC> p;
    constexpr int bytes = TypeInfo<T>::bytes * VEC;
    static_assert(bytes == 4 || bytes == 8 || bytes == 16 || bytes == 32, "packs are 4, 8, 16 or 32 bytes");
    p.zero();
    if (!valid) return p;                                    // uniform: the geometry is the same for every lane
    const uint32_t soff = (uint32_t)y * cx.sHb + (uint32_t)x * cx.sWb;
    if (cx.active) {
        if constexpr (bytes == 16) {
            const sp_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(cx.frame, cx.voff, soff, 0);
            __builtin_memcpy(&p, &v, 16);
        } else if constexpr (bytes == 8) {
            const sp_u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(cx.frame, cx.voff, soff, 0);
            __builtin_memcpy(&p, &v, 8);
        } else if constexpr (bytes == 4) {
            const unsigned v = __builtin_amdgcn_raw_buffer_load_b32(cx.frame, cx.voff, soff, 0);
            __builtin_memcpy(&p, &v, 4);
        } else {
            const sp_u32x4 lo = __builtin_amdgcn_raw_buffer_load_b128(cx.frame, cx.voff, soff, 0);
            const sp_u32x4 hi = __builtin_amdgcn_raw_buffer_load_b128(cx.frame, cx.voff + 16, soff, 0);
            __builtin_memcpy(&p, &lo, 16);
            __builtin_memcpy(reinterpret_cast<char*>(&p) + 16, &hi, 16);
        }
    }
    return p;
}

// the same with the row's byte offset inside the frame already in a scalar register
template <typename T, int VEC>
__device__ __forceinline__ Pack<T, VEC> load_leaf_at(const SpatialCtx& cx, uint32_t soff, bool valid) {
    Pack<T, VEC> p;
    constexpr int bytes = TypeInfo<T>::bytes * VEC;
    p.zero();
    if (!valid) return p;                                    // uniform
    if (cx.active) {
        if constexpr (bytes == 16) {
            const sp_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(cx.frame, cx.voff, soff, 0);
            __builtin_memcpy(&p, &v, 16);
        } else if constexpr (bytes == 8) {
            const sp_u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(cx.frame, cx.voff, soff, 0);
            __builtin_memcpy(&p, &v, 8);
        } else if constexpr (bytes == 4) {
            const unsigned v = __builtin_amdgcn_raw_buffer_load_b32(cx.frame, cx.voff, soff, 0);
            __builtin_memcpy(&p, &v, 4);
        } else {
            const sp_u32x4 lo = __builtin_amdgcn_raw_buffer_load_b128(cx.frame, cx.voff, soff, 0);
            const sp_u32x4 hi = __builtin_amdgcn_raw_buffer_load_b128(cx.frame, cx.voff + 16, soff, 0);
            __builtin_memcpy(&p, &lo, 16);
            __builtin_memcpy(reinterpret_cast<char*>(&p) + 16, &hi, 16);
        }
    }
    return p;
}

// (upstream pooling fused into the leaf load, POOLED: `load_quad_pooled` and the kernel that uses it live in spatial_pooled.inc, included
// only by the translation units that instantiate them; the call below is a dependent name, found at instantiation)
// Request the leaves of a block whose top cell sits at level `lvl` (nothing is consumed here: the loads stay in flight) ...
template <typename T, int VEC, int BL>
__device__ __forceinline__ void load_block(const SpatialCtx& cx, int t, int i, int j, bool valid, const BlockGeo& b, BlockRegs<T, VEC>& r) {
    if constexpr (BL == 1) {
        r.top = load_leaf<T, VEC>(cx, t, i, j, valid);
    } else if constexpr (BL == 2) {
#pragma unroll
        for (int k = 0; k < 4; ++k) r.mid[k] = load_leaf<T, VEC>(cx, t, b.ci[k], b.cj[k], b.v1[k]);
    } else {
        // (one load_leaf per leaf: issuing the sixteen loads back to back from one masked region -- all offsets first -- was
        // measured SLOWER: bf16 C=3584 60.1 -> 62.6 us, 20x36 grids 111 -> 121 us)
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) r.leaf[k][q] = load_leaf<T, VEC>(cx, t, b.li[k][q], b.lj[k][q], b.v2[k][q]);
    }
}
// ... and build mids + top from them.
template <typename T, int VEC, int BL>
__device__ __forceinline__ void pool_block(const SpatialCtx& cx, bool valid, const BlockGeo& b, BlockRegs<T, VEC>& r) {
    if constexpr (BL == 2) {
        r.top = pool4<T, VEC>(r.mid, b.v1, cx.sum_mode);
    } else if constexpr (BL == 3) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (b.v1[k]) r.mid[k] = pool4<T, VEC>(r.leaf[k], b.v2[k], cx.sum_mode);
            else r.mid[k].zero();
        }
        r.top = pool4<T, VEC>(r.mid, b.v1, cx.sum_mode);
    }
    if (!valid) r.top.zero();
}
template <typename T, int VEC, int BL>
__device__ __forceinline__ void load_and_pool_block(const SpatialCtx& cx, int t, int i, int j, bool valid,
                                                    const BlockGeo& b, BlockRegs<T, VEC>& r) {
    load_block<T, VEC, BL>(cx, t, i, j, valid, b, r);
    pool_block<T, VEC, BL>(cx, valid, b, r);
}

// Feature of cell (0,0) of level `lvl` (the alias target of invalid child slots, quirk Q1): pooled from
// scratch with the same arithmetic as the main tree.  LV = levels below `lvl` (0 = leaf level).
template <typename T, int VEC, int LV> struct AliasPool {
    static __device__ __forceinline__ Pack<T, VEC> run(const SpatialCtx& cx, const LevelDims& g, int t, int lvl, int i, int j) {
        const CellGeo c = cell_children(g, lvl, i, j);
        Pack<T, VEC> ch[4];
        bool v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = (k >> 1) < c.rc && (k & 1) < c.cc;
            if (v[k]) ch[k] = AliasPool<T, VEC, LV - 1>::run(cx, g, t, lvl + 1, c.rs + (k >> 1), c.cs + (k & 1));
            else ch[k].zero();
        }
        return pool4<T, VEC>(ch, v, cx.sum_mode);
    }
};
template <typename T, int VEC> struct AliasPool<T, VEC, 0> {
    static __device__ __forceinline__ Pack<T, VEC> run(const SpatialCtx& cx, const LevelDims&, int t, int, int i, int j) {
        return load_leaf<T, VEC>(cx, t, i, j, true);
    }
};

// ---- per-head similarity (sim_per_head / head_dim): cos(p, c) is evaluated per head (G = head_dim / VEC adjacent
// lanes own one head) and averaged over heads (quadtree_builder.py:63-66).  One parent with its four child slots:
// per-thread partial (|P|^2, P.C_k, |C_k|^2) -> sums inside each head group -> per-head ratio on the group leader.
// The caller adds the leaders' ratios over the wave / workgroup and divides by the head count.
template <typename T, int VEC>
__device__ __forceinline__ void head_parent_ratios(const Pack<T, VEC>& P, const Pack<T, VEC> (&C)[4], const bool (&v)[4],
                                                   const Pack<T, VEC>& alias_child, int G, int lane, float (&out)[4]) {
    float np = dot_pack(P, P), d[4], nc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        d[k] = v[k] ? dot_pack(P, C[k]) : dot_pack(P, alias_child);
        nc[k] = v[k] ? dot_pack(C[k], C[k]) : dot_pack(alias_child, alias_child);
    }
    for (int m = 1; m < G; m <<= 1) {
        np += __shfl_xor(np, m, 64);
#pragma unroll
        for (int k = 0; k < 4; ++k) { d[k] += __shfl_xor(d[k], m, 64); nc[k] += __shfl_xor(nc[k], m, 64); }
    }
    const bool leader = (lane & (G - 1)) == 0;
    const float pn = fmaxf(sqrtf(np), 1e-8f);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = leader ? d[k] / (pn * fmaxf(sqrtf(nc[k]), 1e-8f)) : 0.f;
}

// Per-thread partial statistics of one block, transposed-reduced over the wave, accumulated into this
// wave's row of the LDS partial table.  `tn` = tree-node id of the block's top, `lvl` its level.
template <typename T, int VEC, int BL, int D, bool PERHEAD>
__device__ __forceinline__ void block_stats(const BlockRegs<T, VEC>& r, const BlockGeo& b, bool valid, int tn, int lvl,
                                            const Pack<T, VEC> (&alias)[D], float* part, int lane, int G) {
    using TC = TreeConst<D>;
    if constexpr (PERHEAD && BL >= 2) {
        // ratios summed over heads land in the dot slots; norms are not needed in this mode
        if constexpr (BL == 2) {
            float s[4];
            head_parent_ratios<T, VEC>(r.top, r.mid, b.v1, alias[lvl + 1], G, lane, s);
            const float tot = wave_reduce_many<4>(s, lane);
            bool ok;
            const int idx = wave_reduce_slot<4>(lane, ok);
            if (ok && valid) part[TC::dot_id(tn, idx)] = tot;
        } else {
            float s[20];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float o[4];
                head_parent_ratios<T, VEC>(r.mid[k], r.leaf[k], b.v2[k], alias[lvl + 2], G, lane, o);
#pragma unroll
                for (int q = 0; q < 4; ++q) s[k * 4 + q] = b.v1[k] ? o[q] : 0.f;
            }
            {
                float o[4];
                head_parent_ratios<T, VEC>(r.top, r.mid, b.v1, alias[lvl + 1], G, lane, o);
#pragma unroll
                for (int q = 0; q < 4; ++q) s[16 + q] = o[q];
            }
            const float tot = wave_reduce_many<20>(s, lane);
            bool ok;
            const int idx = wave_reduce_slot<20>(lane, ok);
            if (ok && valid) part[idx < 16 ? TC::dot_id(4 * tn + 1 + (idx >> 2), idx & 3) : TC::dot_id(tn, idx - 16)] = tot;
        }
    } else if constexpr (BL == 1) {
        float s[1] = {dot_pack(r.top, r.top)};
        const float tot = wave_reduce_many<1>(s, lane);
        if (lane == 0 && valid) part[tn] = tot;
    } else if constexpr (BL == 2) {
        float s[9];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s[k] = dot_pack(r.mid[k], r.mid[k]);
            s[5 + k] = b.v1[k] ? dot_pack(r.top, r.mid[k]) : dot_pack(r.top, alias[lvl + 1]);
        }
        s[4] = dot_pack(r.top, r.top);
        const float tot = wave_reduce_many<9>(s, lane);
        bool ok;
        const int idx = wave_reduce_slot<9>(lane, ok);
        if (ok && valid) {
            int id;
            if (idx < 4) id = 4 * tn + 1 + idx;
            else if (idx == 4) id = tn;
            else id = TC::dot_id(tn, idx - 5);
            part[id] = tot;
        }
    } else {
        // two mids at a time (18 partials live instead of 41: keeps the kernel at 4 workgroups per CU)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float s[18];
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int k = 2 * h + kk;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    s[kk * 9 + q] = dot_pack(r.leaf[k][q], r.leaf[k][q]);
                    s[kk * 9 + 5 + q] = b.v2[k][q] ? dot_pack(r.mid[k], r.leaf[k][q]) : dot_pack(r.mid[k], alias[lvl + 2]);
                }
                s[kk * 9 + 4] = dot_pack(r.mid[k], r.mid[k]);
            }
            const float tot = wave_reduce_many<18, kSwapStages<T>>(s, lane);
            bool ok;
            const int idx = wave_reduce_slot<18>(lane, ok);
            if (ok && valid) {
                const int k = 2 * h + idx / 9, e = idx % 9;
                const int mid = 4 * tn + 1 + k;
                int id;
                if (e < 4) id = 4 * mid + 1 + e;
                else if (e == 4) id = mid;
                else id = TC::dot_id(mid, e - 5);
                part[id] = tot;
            }
        }
        float s[5];
        s[0] = dot_pack(r.top, r.top);
#pragma unroll
        for (int k = 0; k < 4; ++k) s[1 + k] = b.v1[k] ? dot_pack(r.top, r.mid[k]) : dot_pack(r.top, alias[lvl + 1]);
        const float tot = wave_reduce_many<5, kSwapStages<T>>(s, lane);
        bool ok;
        const int idx = wave_reduce_slot<5>(lane, ok);
        if (ok && valid) part[idx == 0 ? tn : TC::dot_id(tn, idx - 1)] = tot;
    }
}

// store the emitted nodes of a block from registers; orow[node] = destination row in S or -1
template <typename T, int VEC, int BL>
__device__ __forceinline__ void block_store(const BlockRegs<T, VEC>& r, int tn, const int* orow, void* S, int C,
                                            const SpatialCtx& cx, bool skip_leaves) {
    if (!cx.active) return;
    if (BL > 1 || !skip_leaves) {
        const int row = orow[tn];
        if (row >= 0) store_pack<T, VEC>(S, (int64_t)row * C + cx.c0, r.top);
    }
    if constexpr (BL >= 2) {
        if (BL > 2 || !skip_leaves) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int row = orow[4 * tn + 1 + k];
                if (row >= 0) store_pack<T, VEC>(S, (int64_t)row * C + cx.c0, r.mid[k]);
            }
        }
    }
    if constexpr (BL == 3) {
        if (skip_leaves) return;
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = orow[4 * (4 * tn + 1 + k) + 1 + q];
                if (row >= 0) store_pack<T, VEC>(S, (int64_t)row * C + cx.c0, r.leaf[k][q]);
            }
    }
}

// Locate tree node n below root cell (I, J): depth, cell coordinates, validity, and the ids on its path.
struct NodeLoc {
    int depth, i, j;
    bool valid;
    int path[kMaxLevels];     // node ids from the root (path[0] = 0) down to the node itself
    int slot[kMaxLevels];     // slot[d] = child slot taken to reach depth d (slot[0] unused)
    int pi[kMaxLevels], pj[kMaxLevels];   // cell coordinates along the path
};
__device__ __forceinline__ NodeLoc locate(const LevelDims& g, int I, int J, int n) {
    NodeLoc L;
    int d = 0;
    while (depth_base(d + 1) <= n) ++d;
    L.depth = d;
    const int rel = n - depth_base(d);
    L.i = I; L.j = J; L.valid = true;
    L.path[0] = 0; L.pi[0] = I; L.pj[0] = J;
    int id = 0;
    for (int s = 1; s <= d; ++s) {
        const int k = (rel >> (2 * (d - s))) & 3;
        const CellGeo c = cell_children(g, s - 1, L.i, L.j);
        if ((k >> 1) >= c.rc || (k & 1) >= c.cc) L.valid = false;
        L.i = c.rs + (k >> 1);
        L.j = c.cs + (k & 1);
        id = 4 * id + 1 + k;
        L.path[s] = id;
        L.slot[s] = k;
        if (!L.valid) { L.i = 0; L.j = 0; }
        L.pi[s] = L.i; L.pj[s] = L.j;
    }
    return L;
}

// F.cosine_similarity(p, c) = sum((p / max(|p|, eps)) * (c / max(|c|, eps))), eps = 1e-8, then `>= threshold` on
// the fp32 value (quadtree_builder.py:61-68).  With the fp32 sums dot, |p|^2, |c|^2 the test
//     fp32(dot / (max(|p|,eps) * max(|c|,eps))) >= thr
// is evaluated without sqrt/div: rounding to fp32 is monotonic, so it equals  sim >= lo  where lo is the smallest
// real that rounds to >= thr (`thr_lo`, computed on the host in double), and  sim >= lo  <=>
// dot*|dot| >= lo*|lo| * max(|p|^2, eps^2) * max(|c|^2, eps^2)   (the product of two fp32 values is exact in double).
// A sum of squares that is +inf (an Inf element, or finite elements whose squares overflow fp32) would turn the test into
// inf >= inf.  The reference divides every element by max(|x|, eps) = inf there: NaN when an element is Inf (inf / inf; dot is
// then +-inf or NaN as well), 0 when only the norm overflowed -- never >= a positive threshold, and 0 >= lo for lo <= 0 only while
// dot is finite (an infinite dot with lo <= 0 cannot be told apart from the sums alone and counts as the NaN case).
// A NaN element needs nothing extra: fmax drops the NaN norm but dot is NaN, and NaN >= x is false.
__device__ __forceinline__ bool cosine_at_least(float dot, float n2a, float n2b, double lo_sq_signed) {
    const double a = fmax((double)n2a, 1e-16), b = fmax((double)n2b, 1e-16);
    const double d = (double)dot, ab = a * b;
    if (!(ab < HUGE_VAL)) return lo_sq_signed <= 0.0 && fabs(d) < HUGE_VAL;
    return d * fabs(d) >= lo_sq_signed * ab;
}

// Same as locate() for a node whose depth DEPTH is known at compile time: every loop unrolls, the per-level
// arrays are register-allocated (the generic version indexes them dynamically and lands in scratch memory).
template <int DEPTH>
__device__ __forceinline__ NodeLoc locate_static(const LevelDims& g, int I, int J, int rel) {
    NodeLoc L;
    L.depth = DEPTH;
    L.i = I; L.j = J; L.valid = true;
    L.path[0] = 0; L.pi[0] = I; L.pj[0] = J; L.slot[0] = 0;
    int id = 0;
#pragma unroll
    for (int s = 1; s <= DEPTH; ++s) {
        const int k = (rel >> (2 * (DEPTH - s))) & 3;
        const CellGeo c = cell_children(g, s - 1, L.i, L.j);
        if ((k >> 1) >= c.rc || (k & 1) >= c.cc) L.valid = false;
        L.i = c.rs + (k >> 1);
        L.j = c.cs + (k & 1);
        id = 4 * id + 1 + k;
        L.path[s] = id;
        L.slot[s] = k;
        if (!L.valid) { L.i = 0; L.j = 0; }
        L.pi[s] = L.i; L.pj[s] = L.j;
    }
    return L;
}

// one (parent, slot) cosine test for parents of a compile-time depth
template <int D, int DEPTH, bool PERHEAD>
__device__ __forceinline__ void parent_slot_test(const SpatialArgs& a, int I, int J, int rel, int k, const float* stat, int* stop) {
    using TC = TreeConst<D>;
    const NodeLoc L = locate_static<DEPTH>(a.dims, I, J, rel);
    if (!L.valid) return;
    const int p = depth_base(DEPTH) + rel;
    const CellGeo c = cell_children(a.dims, DEPTH, L.i, L.j);
    const bool vk = (k >> 1) < c.rc && (k & 1) < c.cc;
    if constexpr (PERHEAD) {
        // the dot slot holds the sum over heads of the per-head cosines: mean >= threshold (quadtree_builder.py:66-68)
        if (!(stat[TC::dot_id(p, k)] / (float)a.n_head >= a.threshold)) stop[p] = 0;
    } else {
        const float n2c = vk ? stat[4 * p + 1 + k] : stat[TC::alias_id(DEPTH + 1)];
        if (!cosine_at_least(stat[TC::dot_id(p, k)], stat[p], n2c, a.thr_lo_sq)) stop[p] = 0;
    }
}

// Phases 2-4 of one (frame, root cell) item, entered after the per-wave partial statistics are in LDS and a
// barrier: fixed-order cross-wave sums, every (parent, slot) cosine test + every node's inverse norm in parallel,
// then one thread per leaf position emits.  Ends with a barrier; orow[] then maps tree node -> row in S (or -1).
template <int D, bool PERHEAD>
__device__ __forceinline__ void decide_and_emit(const SpatialArgs& a, int t, int I, int J, int item, const float* part,
                                                float* stat, int* stop, int* orow, int* lcount, double* inrm_l, int nwave) {
    using TC = TreeConst<D>;
    constexpr int NSTAT = TC::NSTAT;
    const LevelDims& g = a.dims;
    const int tid = threadIdx.x;
    const int HW = a.H * a.W;
    int* rc_list = a.rc_list + (int64_t)item * a.rc_stride;
    // ---- phase 2: cross-wave sum in a fixed order ------------------------------------------------------------
    for (int s2 = tid; s2 < NSTAT; s2 += blockDim.x) {
        float acc = 0.f;
        for (int w = 0; w < nwave; ++w) acc += part[w * NSTAT + s2];
        stat[s2] = acc;
    }
    lds_barrier();         // every hand-over of this function goes through LDS: global traffic may stay in flight
    // ---- phase 3: every (parent, slot) cosine test and every node's inverse norm, one thread each, spread over
    //      the waves so the four SIMDs work side by side -----------------------------------------------------------
    // Every KIND of item starts at a wave boundary of its own: the tests of the parents of one depth (table walks of that depth), the
    // inverse norms (a double-precision sqrt + divide).  They are different code, and lanes of ONE wave would run them one after
    // the other (round 3: all 41 items of a 3-level tree sat in wave 0 -- 0.7 us of the kernel).  Waves without an item skip the
    // phase (execz branches).  kind_first(c) = first thread of kind c, modulo the block size.
    {
        const int bd = (int)blockDim.x;
        auto mine = [&](int first, int count, auto&& fn) {           // items first .. first + count - 1 -> threads (first + i) % bd
            const int f = first % bd;
            for (int i = tid >= f ? tid - f : tid + bd - f; i < count; i += bd) fn(i);
        };
        int first = 0;
        if constexpr (D <= 3) {
            if constexpr (D >= 2) { mine(first, 4 * pow4(0), [&](int e) { parent_slot_test<D, 0, PERHEAD>(a, I, J, e >> 2, e & 3, stat, stop); }); first += (4 * pow4(0) + 63) & ~63; }
            if constexpr (D >= 3) { mine(first, 4 * pow4(1), [&](int e) { parent_slot_test<D, 1, PERHEAD>(a, I, J, e >> 2, e & 3, stat, stop); }); first += (4 * pow4(1) + 63) & ~63; }
        } else {
            // deeper trees: all tests share the first wave(s) -- a wave per depth was measured slower there (20 x 36 grids, 4 levels:
            // 107.9 -> 113.2 us; every wave of the workgroup then steps through the phase)
            mine(first, 4 * TC::NPAR, [&](int e) {
                const int p = e >> 2, k = e & 3;
                if (p < depth_base(1)) parent_slot_test<D, 0, PERHEAD>(a, I, J, p, k, stat, stop);
                else if (p < depth_base(2)) parent_slot_test<D, 1, PERHEAD>(a, I, J, p - depth_base(1), k, stat, stop);
                else if (p < depth_base(3)) parent_slot_test<D, 2, PERHEAD>(a, I, J, p - depth_base(2), k, stat, stop);
                else if constexpr (D >= 5) {
                    if (p < depth_base(4)) parent_slot_test<D, 3, PERHEAD>(a, I, J, p - depth_base(3), k, stat, stop);
                    else if constexpr (D >= 6) parent_slot_test<D, 4, PERHEAD>(a, I, J, p - depth_base(4), k, stat, stop);
                }
            });
            first += (4 * TC::NPAR + 63) & ~63;
        }
        mine(first, TC::NNODE, [&](int n) { inrm_l[n] = 1.0 / (sqrt((double)stat[n]) + 1e-8); });      // temporal stage: x / (|x| + 1e-8)
    }
    lds_barrier();
    // ---- phase 4: emission, one thread per leaf position of the root cell -------------------------------------
    // The leaf-level node learns its first stopped ancestor (or itself): that node is emitted; the leaf that is its
    // top-left descendant (all slots below it are 0) is the node's origin and writes the node's metadata.
    for (int q = tid; q < TC::NLEAF; q += blockDim.x) {
        const NodeLoc L = locate_static<D - 1>(g, I, J, q);
        if (!L.valid) continue;
        int da = D - 1;
#pragma unroll
        for (int d = D - 2; d >= 0; --d) {
            if (stop[L.path[d]]) da = d;                       // ends at the SHALLOWEST stopped ancestor
        }
        bool origin = true;
        int emit_node = L.path[D - 1], hi_i = L.i, hi_j = L.j;
#pragma unroll
        for (int d = D - 1; d >= 0; --d) {
            if (d > da) origin = origin && (L.slot[d] == 0);
            if (d == da) { emit_node = L.path[d]; hi_i = L.pi[d]; hi_j = L.pj[d]; }
        }
        const int leaf_row = t * HW + L.i * a.W + L.j;
        if (t == 0) {
            // the root cell's geometry, once per leaf position (the group-mean kernel maps column slots to rows with it)
            int lo_i = I, hi_i = I, lo_j = J, hi_j = J;
#pragma unroll
            for (int m = 0; m < D - 1; ++m) {
                lo_i = child_start(lo_i, g.h[m + 1]);
                hi_i = child_start(hi_i, g.h[m + 1]) + child_count(hi_i, g.h[m + 1]) - 1;
                lo_j = child_start(lo_j, g.w[m + 1]);
                hi_j = child_start(hi_j, g.w[m + 1]) + child_count(hi_j, g.w[m + 1]) - 1;
            }
            a.cgeo[L.i * a.W + L.j] = (uint32_t)lo_i | ((uint32_t)lo_j << 8) | ((uint32_t)(hi_j - lo_j + 1) << 16) | ((uint32_t)(hi_i - lo_i + 1) << 24);
        }
        // defaults for the temporal stage: every node is its own representative with a group of one (only nodes with a kept
        // cross-frame edge are touched again by the label stage)
        if (!origin) { a.meta[leaf_row] = 0u; a.lab_row[leaf_row] = -1; a.gcnt[leaf_row] = 0; continue; }
        // box of the emitted ancestor: top-left is this leaf; bottom-right follows last children down
#pragma unroll
        for (int m = 0; m < D - 1; ++m) {
            if (m >= da) {
                hi_i = child_start(hi_i, g.h[m + 1]) + child_count(hi_i, g.h[m + 1]) - 1;
                hi_j = child_start(hi_j, g.w[m + 1]) + child_count(hi_j, g.w[m + 1]) - 1;
            }
        }
        const int y2 = hi_i + 1, x2 = hi_j + 1;
        a.meta[leaf_row] = ((uint32_t)y2 << 16) | (uint32_t)x2;
        a.inrm[leaf_row] = inrm_l[emit_node];
        a.lab_row[leaf_row] = leaf_row;
        a.gcnt[leaf_row] = 1;
        orow[emit_node] = leaf_row;
        const int pos = atomicAdd(lcount, 1);
        if (y2 - L.i == 1 && x2 - L.j == 1) atomicAdd(lcount + 1, 1);
        rc_list[1 + pos] = (L.i << 24) | (L.j << 16) | (y2 << 8) | x2;
    }
    lds_barrier();         // orow / lcount live in LDS; the metadata stores above stay in flight under the node stores
    if (tid == 0) {
        rc_list[0] = lcount[0] | (lcount[1] << 16);          // nodes | 1x1 nodes of this (frame, root cell)
        if (I == 0 && J == 0) a.frame_cnt[t] = 0;            // consumed (atomically) by the label stage
    }
    if (item == 0) {                                         // the counters of the later kernels
        if (tid < STTM_CNT_SLOTS) a.counts[tid] = 0;
        if (tid < 8) a.bar[tid] = 0;
        const int R = g.h[0] * g.w[0];
        for (int i = tid; i < R; i += blockDim.x) a.col_arrive[i] = 0;
    }
}

// ---- trees with three or more levels above the register blocks (UL >= 3).  The upper levels are a recursion over the level
// (compile time) with RUN-TIME loops over the four children, so the block code exists once per phase instead of 4^UL times;
// child results are kept in registers through compile-time-indexed selects.
template <typename T, int VEC>
__device__ __forceinline__ void keep_child(Pack<T, VEC> (&ch)[4], bool (&v)[4], int k, const Pack<T, VEC>& r, bool valid) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
        if (kk == k) { ch[kk] = r; v[kk] = valid; }
}
// upper_cell: feature of cell (i, j) of level `lvl` (tree node tn), with the statistics of everything below it accumulated into
// this wave's partial table.  UREM = levels between this cell and the block tops (0: the cell IS a block top).
template <typename T, int VEC, int BL, int D, int UREM, bool PERHEAD>
__device__ __forceinline__ Pack<T, VEC> upper_cell(const SpatialCtx& cx, const LevelDims& g, int t, int lvl, int i, int j, int tn,
                                                   const Pack<T, VEC> (&alias)[D], float* mypart, int lane, int head_lanes,
                                                   BlockRegs<T, VEC>& regs, BlockGeo& bg) {
    using TC = TreeConst<D>;
    if constexpr (UREM == 0) {
        block_geometry<BL>(g, lvl, i, j, true, bg);
        load_and_pool_block<T, VEC, BL>(cx, t, i, j, true, bg, regs);
        block_stats<T, VEC, BL, D, PERHEAD>(regs, bg, true, tn, lvl, alias, mypart, lane, head_lanes);
        return regs.top;
    } else {
        const CellGeo c = cell_children(g, lvl, i, j);
        Pack<T, VEC> ch[4];
        bool v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { ch[k].zero(); v[k] = false; }
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            if ((k >> 1) < c.rc && (k & 1) < c.cc) {
                const Pack<T, VEC> r = upper_cell<T, VEC, BL, D, UREM - 1, PERHEAD>(cx, g, t, lvl + 1, c.rs + (k >> 1), c.cs + (k & 1),
                                                                                     4 * tn + 1 + k, alias, mypart, lane, head_lanes, regs, bg);
                keep_child<T, VEC>(ch, v, k, r, true);
            }
        }
        const Pack<T, VEC> me = pool4<T, VEC>(ch, v, cx.sum_mode);
        // alias[] is indexed by a run-time level here: select with compile-time indices
        Pack<T, VEC> al;
        al.zero();
#pragma unroll
        for (int m = 1; m < D; ++m)
            if (m == lvl + 1) al = alias[m];
        if constexpr (PERHEAD) {
            float s[4];
            head_parent_ratios<T, VEC>(me, ch, v, al, head_lanes, lane, s);
            const float tot = wave_reduce_many<4>(s, lane);
            bool ok;
            const int idx = wave_reduce_slot<4>(lane, ok);
            if (ok) mypart[TC::dot_id(tn, idx)] = tot;
        } else {
            float s[5];
            s[0] = dot_pack(me, me);
#pragma unroll
            for (int k = 0; k < 4; ++k) s[1 + k] = v[k] ? dot_pack(me, ch[k]) : dot_pack(me, al);
            const float tot = wave_reduce_many<5>(s, lane);
            bool ok;
            const int idx = wave_reduce_slot<5>(lane, ok);
            if (ok) mypart[idx == 0 ? tn : TC::dot_id(tn, idx - 1)] = tot;
        }
        return me;
    }
}
// the same pooling without statistics (store phase: the feature of a stopped upper cell is rebuilt from the L2-resident leaves)
template <typename T, int VEC, int BL, int UREM>
__device__ __forceinline__ Pack<T, VEC> pooled_cell(const SpatialCtx& cx, const LevelDims& g, int t, int lvl, int i, int j,
                                                    BlockRegs<T, VEC>& regs, BlockGeo& bg) {
    if constexpr (UREM == 0) {
        block_geometry<BL>(g, lvl, i, j, true, bg);
        load_and_pool_block<T, VEC, BL>(cx, t, i, j, true, bg, regs);
        return regs.top;
    } else {
        const CellGeo c = cell_children(g, lvl, i, j);
        Pack<T, VEC> ch[4];
        bool v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { ch[k].zero(); v[k] = false; }
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            if ((k >> 1) < c.rc && (k & 1) < c.cc) {
                const Pack<T, VEC> r = pooled_cell<T, VEC, BL, UREM - 1>(cx, g, t, lvl + 1, c.rs + (k >> 1), c.cs + (k & 1), regs, bg);
                keep_child<T, VEC>(ch, v, k, r, true);
            }
        }
        return pool4<T, VEC>(ch, v, cx.sum_mode);
    }
}
// store phase below cell tn (whose ancestors all split): a stopped cell is the emitted node, otherwise descend; block tops and
// everything inside a block are handled by block_store after re-reading the block
template <typename T, int VEC, int BL, int UREM>
__device__ __forceinline__ void store_cell(const SpatialCtx& cx, const LevelDims& g, int t, int lvl, int i, int j, int tn,
                                           const int* stop, const int* orow, void* S, int C, bool leaves_in_x,
                                           BlockRegs<T, VEC>& regs, BlockGeo& bg) {
    if constexpr (UREM == 0) {
        block_geometry<BL>(g, lvl, i, j, true, bg);
        load_and_pool_block<T, VEC, BL>(cx, t, i, j, true, bg, regs);
        block_store<T, VEC, BL>(regs, tn, orow, S, C, cx, leaves_in_x);
    } else {
        if (stop[tn]) {
            const Pack<T, VEC> me = pooled_cell<T, VEC, BL, UREM>(cx, g, t, lvl, i, j, regs, bg);
            if (cx.active && orow[tn] >= 0) store_pack<T, VEC>(S, (int64_t)orow[tn] * C + cx.c0, me);
            return;
        }
        const CellGeo c = cell_children(g, lvl, i, j);
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            if ((k >> 1) < c.rc && (k & 1) < c.cc)
                store_cell<T, VEC, BL, UREM - 1>(cx, g, t, lvl + 1, c.rs + (k >> 1), c.cs + (k & 1), 4 * tn + 1 + k, stop, orow, S, C,
                                                 leaves_in_x, regs, bg);
        }
    }
}

#define STTM_K1_TICK(n) STTM_DEV_TICK(a.dev, k1_ticks, blockIdx.x == a.dev.k1_wg, n)
#ifdef STTM_DEV
#define STTM_K1_END() \
    do { \
        if (a.dev.k1_span && threadIdx.x == 0) a.dev.k1_span[2 * wg + 1] = wall_clock64(); \
        if (a.dev.k1_mode >= 10) {           /* experiment: (k1_mode - 10) microseconds of latency-bound tail work per workgroup */ \
            const long long t0_ = wall_clock64(); \
            while (wall_clock64() - t0_ < (long long)(a.dev.k1_mode - 10) * 100) __builtin_amdgcn_s_sleep(2); \
        } \
    } while (0)
#else
#define STTM_K1_END() do { } while (0)
#endif

// ---------------------------------------------------------------------------------------------------
// Root cells of a 3-level tree (round 4; every run_vidqa.sh preset: 14 x 14 / root_level 1).  The whole (frame, root cell) item
// as ONE shape -- top, 4 mids, 16 leaf slots -- in two instantiations picked by a SCALAR branch:
//   FULL  = every child and grandchild exists (a workgroup-uniform fact known from blockIdx: 9 of the 16 root cells of a
//           14 x 14 frame = 144 of its 196 leaves, every cell of an even pyramid): all validity flags are compile-time
//           constants, the pooled sums and the 41 statistics are straight-line code, the leaf rows are y0 .. y0+3 x x0 .. x0+3;
//   !FULL = cells that own the lone first row / column of an odd level.  Missing slots are FILLED WITH THEIR ALIAS (quirk Q1:
//           an invalid child slot of a parent at level l is compared with cell (t, 0, 0) of level l+1): a missing leaf slot
//           loads leaf (0, 0); the four leaf slots of a missing mid load the leaves of mid (0, 0), whose pooled feature lands in
//           that mid's registers.  The statistics then need no selects at all -- parent . alias and |alias|^2 appear in the slot's
//           own positions -- and only the pooled sums look at (uniform) validity flags.  The alias packs, their norms and
//           their separate loads + pooling of the general body are gone.
// Both: every wave writes all 41 partial sums (no LDS clearing, no barrier before the statistics), and the decisions need no
// LDS tables, no atomics and no further barrier: after the ONE barrier behind the statistics every wave sums the per-wave
// partials itself (lane s <-> statistic s, fixed order over the waves), lanes 0..19 evaluate the 20 (parent, slot) tests with
// the division-free double test, one ballot gives the 20-bit result and the five stop flags are SCALAR bit tests of it.
// Wave 0's lanes 0..15 <-> the sixteen leaf slots write the metadata (positions in the node list through ballots); every
// wave stores its channels of the emitted pooled nodes under scalar branches.
// ---------------------------------------------------------------------------------------------------
struct AxisGeo {          // one axis of a 3-level root cell: leaf offset of (mid d, leaf e) = (d ? cnt0 : 0) + e
    int lo;               // first leaf row / column
    int n_mid;            // mids along the axis (1 or 2)
    int cnt0;             // leaves of the first mid along the axis (1 or 2; a second mid always has 2)
    int acnt;             // leaves of mid 0 of the LEVEL along the axis (the alias cell's extent)
};
template <bool FULL>
__device__ __forceinline__ AxisGeo axis_geo(int i, int n1, int n2) {
    AxisGeo g;
    if constexpr (FULL) {
        g.lo = 2 * (2 * i - (n1 & 1)) - (n2 & 1);          // i is not the lone first cell of an odd level
        g.n_mid = 2; g.cnt0 = 2; g.acnt = 2;
    } else {
        const int m0 = child_start(i, n1);
        g.lo = child_start(m0, n2);
        g.n_mid = child_count(i, n1);
        g.cnt0 = child_count(m0, n2);
        g.acnt = child_count(0, n2);
    }
    return g;
}

// SPLIT (deep trees over several workgroups, below): the item is one 3-level BLOCK of a deeper root cell -- `a.dims` holds the block
// level and the two levels under it --; the node lists, the root-cell geometry and the counters belong to the pass over the upper
// levels (k_spatial_upper), which also gets the block's top through `tops`.
template <typename T, int VEC, bool FULL, bool SPLIT = false, bool POOLED = false>
__device__ __forceinline__ void spatial_block3(const SpatialArgs& a, const SpatialCtx& cx, int t, int I, int J, int item,
                                               float* part, int nwave, void* tops = nullptr) {
    using TC = TreeConst<3>;
    constexpr int NSTAT = TC::NSTAT;
    const LevelDims& g = a.dims;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    const AxisGeo gy = axis_geo<FULL>(I, g.h[1], g.h[2]), gx = axis_geo<FULL>(J, g.w[1], g.w[2]);
    // ---- the sixteen leaf slots, requested before anything else ------------------------------------------------------------
    // Row offsets are formed with integer arithmetic on 0 / 1 flags and pinned to scalar registers (readfirstlane): a select on
    // a uniform bool is a v_cndmask to the compiler, and a vector offset turns every buffer load into a waterfall loop.
    BlockRegs<T, VEC> r;
    bool v1[4], pv[4][4];          // mid k exists | leaf slot (k, q) takes part in the pooled sum of mid register k
    unsigned vleaf = 0;            // bit 4k+q: leaf slot (k, q) is a leaf of this root cell
    const uint32_t soff0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)gy.lo * cx.sHb + (uint32_t)gx.lo * cx.sWb));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int dy = k >> 1, dx = k & 1;
        const int v1i = FULL ? 1 : ((dy < gy.n_mid) & (dx < gx.n_mid));
        v1[k] = v1i != 0;
        int py[4], px[4];
        bool pvalid[4];
        (void)py; (void)px; (void)pvalid;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ey = q >> 1, ex = q & 1;
            if constexpr (FULL) {
                pv[k][q] = true;
                if constexpr (POOLED) { py[q] = gy.lo + 2 * dy + ey; px[q] = gx.lo + 2 * dx + ex; pvalid[q] = true; }
                else r.leaf[k][q] = load_leaf_at<T, VEC>(cx, soff0 + (uint32_t)(2 * dy + ey) * cx.sHb + (uint32_t)(2 * dx + ex) * cx.sWb, true);
            } else {
                const int own = v1i & (ey < (dy ? 2 : gy.cnt0)) & (ex < (dx ? 2 : gx.cnt0));
                const int amid = (v1i ^ 1) & (ey < gy.acnt) & (ex < gx.acnt);           // a leaf of mid (0, 0), the alias of a missing mid
                pv[k][q] = (own | amid) != 0;
                vleaf |= (unsigned)own << (4 * k + q);
                // own leaf | leaf of the alias mid | (missing leaf of an existing mid) the alias leaf (0, 0) | nothing
                const int y = own * (gy.lo + (dy ? gy.cnt0 : 0) + ey) + amid * ey;
                const int x = own * (gx.lo + (dx ? gx.cnt0 : 0) + ex) + amid * ex;
                if constexpr (POOLED) {
                    py[q] = y; px[q] = x; pvalid[q] = (own | amid | v1i) != 0;
                } else {
                    const uint32_t soff = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)y * cx.sHb + (uint32_t)x * cx.sWb));
                    r.leaf[k][q] = load_leaf_at<T, VEC>(cx, soff, (own | amid | v1i) != 0);
                }
            }
        }
        if constexpr (POOLED) load_quad_pooled(cx, py, px, pvalid, r.leaf[k]);
    }
    if constexpr (FULL) vleaf = 0xffffu;
    // ---- pyramid + statistics ------------------------------------------------------------------------------------------------
#pragma unroll
    for (int k = 0; k < 4; ++k) r.mid[k] = pool4<T, VEC>(r.leaf[k], pv[k], cx.sum_mode);
    r.top = pool4<T, VEC>(r.mid, v1, cx.sum_mode);
    STTM_K1_TICK(1);
#ifdef STTM_DEV
    if (a.dev.k1_mode == 2) {               // ablation: loads + pooling only (one store keeps them alive)
        if (cx.active) store_pack<T, VEC>(a.S, (int64_t)item * a.C + cx.c0, r.top);
        return;
    }
#endif
    {
        BlockGeo all;                       // every slot carries what its statistic needs: no selects
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            all.v1[k] = true;
#pragma unroll
            for (int q = 0; q < 4; ++q) all.v2[k][q] = true;
        }
        Pack<T, VEC> unused[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) unused[m].zero();
        block_stats<T, VEC, 3, 3, false>(r, all, true, 0, 0, unused, part + wave * NSTAT, lane, 0);
    }
    lds_barrier();
    STTM_K1_TICK(2);
#ifdef STTM_DEV
    if (a.dev.k1_mode == 1) return;
#endif
    // ---- decisions, every wave for itself ------------------------------------------------------------------------------------
    float st = 0.f;
    {
        const int s = lane < TC::NNODE + 4 * TC::NPAR ? lane : 0;
        for (int w = 0; w < nwave; ++w) st += part[w * NSTAT + s];
    }
    // test e = (parent p = e >> 2, slot k = e & 3): dot = stat[NNODE + e], |p|^2 = stat[p], |c|^2 = stat[4p + 1 + k] = stat[e + 1]
    // (a missing slot holds its alias, so it is tested like the reference tests it; tests of a missing mid are never looked at)
    const int e = lane < 4 * TC::NPAR ? lane : 0;
    const float dot = __shfl(st, TC::NNODE + e, 64), n2p = __shfl(st, e >> 2, 64), n2c = __shfl(st, e + 1, 64);
    const bool pass = lane < 4 * TC::NPAR && cosine_at_least(dot, n2p, n2c, a.thr_lo_sq);
    const unsigned passed = (unsigned)__ballot(pass);
    bool stop[5];
#pragma unroll
    for (int p = 0; p < 5; ++p) stop[p] = ((passed >> (4 * p)) & 15u) == 15u;
    // ---- metadata: wave 0, lane <-> leaf slot (k = lane >> 2, q = lane & 3) -------------------------------------------------
    const int HW = a.H * a.W;
    const int rh = gy.cnt0 + (gy.n_mid - 1) * 2, rw = gx.cnt0 + (gx.n_mid - 1) * 2;      // leaf extent of the root cell
    if (wave == 0) {
        const int k = (lane >> 2) & 3, q = lane & 3;
        const int dy = k >> 1, dx = k & 1;
        const int my = gy.lo + (dy ? gy.cnt0 : 0), mx = gx.lo + (dx ? gx.cnt0 : 0);      // first leaf of mid k
        const int y = my + (q >> 1), x = mx + (q & 1);
        const int leaf_row = t * HW + y * a.W + x;
        const bool mine = lane < 16 && ((vleaf >> (lane & 15)) & 1u);
        bool stop_mid = false;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
            if (kk == k) stop_mid = stop[1 + kk];
        // the emitted ancestor of this leaf (shallowest stopped one), whether this leaf is its origin, its box
        int emit_node, y2, x2;
        bool origin;
        if (stop[0]) { emit_node = 0; origin = k == 0 && q == 0; y2 = gy.lo + rh; x2 = gx.lo + rw; }
        else if (stop_mid) { emit_node = 1 + k; origin = q == 0; y2 = my + (dy ? 2 : gy.cnt0); x2 = mx + (dx ? 2 : gx.cnt0); }
        else { emit_node = 5 + 4 * k + q; origin = true; y2 = y + 1; x2 = x + 1; }
        const float n2 = __shfl(st, emit_node, 64);
        const unsigned long long om = __ballot(mine && origin), o1 = __ballot(mine && origin && y2 - y == 1 && x2 - x == 1);      // (a lone mid / top is a 1x1 node too)
        if (mine) {
            if constexpr (!SPLIT)
                if (t == 0) a.cgeo[y * a.W + x] = (uint32_t)gy.lo | ((uint32_t)gx.lo << 8) | ((uint32_t)rw << 16) | ((uint32_t)rh << 24);
            if (origin) {
                a.meta[leaf_row] = ((uint32_t)y2 << 16) | (uint32_t)x2;
                a.inrm[leaf_row] = 1.0 / (sqrt((double)n2) + 1e-8);          // temporal stage: x / (|x| + 1e-8)
                a.lab_row[leaf_row] = leaf_row;
                a.gcnt[leaf_row] = 1;
                if constexpr (!SPLIT) {
                    int* rc_list = a.rc_list + (int64_t)item * a.rc_stride;
                    rc_list[1 + __popcll(om & ((1ull << lane) - 1ull))] = (y << 24) | (x << 16) | (y2 << 8) | x2;
                    if (lane == 0) rc_list[0] = __popcll(om) | (__popcll(o1) << 16);       // slot (0, 0) always exists and is an origin
                }
            } else {
                a.meta[leaf_row] = 0u; a.lab_row[leaf_row] = -1; a.gcnt[leaf_row] = 0;
            }
        }
        if constexpr (!SPLIT)
            if (tid == 0 && I == 0 && J == 0) a.frame_cnt[t] = 0;            // consumed (atomically) by the label stage
    }
    if constexpr (!SPLIT) {
        if (item == 0) {                                         // the counters of the later kernels
            if (tid < STTM_CNT_SLOTS) a.counts[tid] = 0;
            if (tid < 8) a.bar[tid] = 0;
            const int R = g.h[0] * g.w[0];
            for (int i = tid; i < R; i += blockDim.x) a.col_arrive[i] = 0;
        }
    }
    STTM_K1_TICK(3);
    // ---- features of the emitted pooled nodes, straight from registers (1x1 nodes of a dense input stay in x) -----------------
    if (!cx.active) return;
    if constexpr (SPLIT) store_pack<T, VEC>(tops, (int64_t)item * a.C + cx.c0, r.top);        // tops[t][I][J]: item = t * blocks + I * w + J
    const int64_t row0 = (int64_t)t * HW + (int64_t)gy.lo * a.W + gx.lo;
    if (stop[0]) {
        if (rh * rw > 1 || !a.leaves_in_x) store_pack<T, VEC>(a.S, row0 * a.C + cx.c0, r.top);
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!v1[k]) continue;
        const int dy = k >> 1, dx = k & 1;
        const int mh = dy ? 2 : gy.cnt0, mw = dx ? 2 : gx.cnt0;
        const int64_t rowk = row0 + (int64_t)(dy ? gy.cnt0 : 0) * a.W + (dx ? gx.cnt0 : 0);
        if (stop[1 + k]) {
            if (mh * mw > 1 || !a.leaves_in_x) store_pack<T, VEC>(a.S, rowk * a.C + cx.c0, r.mid[k]);
        } else if (!a.leaves_in_x) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if ((q >> 1) < mh && (q & 1) < mw)
                    store_pack<T, VEC>(a.S, (rowk + (int64_t)(q >> 1) * a.W + (q & 1)) * a.C + cx.c0, r.leaf[k][q]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Root cells of a 4-level tree (round 4; the Qwen2-VL grids of BASELINE config 4 at root_level 1: 20 x 36, 18 x 26, also 27 x 27):
// the root over up to four 3-level blocks, each handled like spatial_block3's general instantiation -- sixteen leaf slots, missing
// slots filled with their alias, statistics without selects -- in a run-time loop over the block slots (one copy of the block
// code).  A MISSING BLOCK SLOT holds the alias of its level, block (0, 0) of level 1, whose top is what the root is compared with
// there.  Only the four block tops and the root stay in registers; a block whose interior is emitted is re-read for the store
// phase (L2-resident) -- when the root or the block top stops, which is the common case on these grids, nothing is re-read.
// Decisions: 84 (parent, slot) tests in two ballot passes over per-wave statistic sums kept in LDS (wave-private: no barrier);
// metadata: wave 0, lane <-> one of the 64 leaf slots.  The general body (k1_var = 1, development build) carried 1 470 selects,
// 1 586 scalar-spill reloads and four barriers for these trees.
// ---------------------------------------------------------------------------------------------------
struct Block3Shape {
    AxisGeo gy, gx;
    unsigned v1m;        // bit k: mid k exists
    unsigned vleaf;      // bit 4k+q: leaf slot (k, q) is a leaf of the block
};
// loads + pools one block whose top is cell (bi, bj) of the level above `n1` (n1 / n2 = cells per axis of the block's mid / leaf level)
template <typename T, int VEC>
__device__ __forceinline__ Block3Shape block3_unit(const SpatialCtx& cx, int bi, int bj, int h1, int w1, int h2, int w2, BlockRegs<T, VEC>& r) {
    Block3Shape sh;
    sh.gy = axis_geo<false>(bi, h1, h2);
    sh.gx = axis_geo<false>(bj, w1, w2);
    const AxisGeo& gy = sh.gy; const AxisGeo& gx = sh.gx;
    bool v1[4], pv[4][4];
    sh.v1m = 0; sh.vleaf = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int dy = k >> 1, dx = k & 1;
        const int v1i = (dy < gy.n_mid) & (dx < gx.n_mid);
        v1[k] = v1i != 0;
        sh.v1m |= (unsigned)v1i << k;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ey = q >> 1, ex = q & 1;
            const int own = v1i & (ey < (dy ? 2 : gy.cnt0)) & (ex < (dx ? 2 : gx.cnt0));
            const int amid = (v1i ^ 1) & (ey < gy.acnt) & (ex < gx.acnt);           // a leaf of mid (0, 0), the alias of a missing mid
            pv[k][q] = (own | amid) != 0;
            sh.vleaf |= (unsigned)own << (4 * k + q);
            const int y = own * (gy.lo + (dy ? gy.cnt0 : 0) + ey) + amid * ey;
            const int x = own * (gx.lo + (dx ? gx.cnt0 : 0) + ex) + amid * ex;
            const uint32_t soff = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)y * cx.sHb + (uint32_t)x * cx.sWb));
            r.leaf[k][q] = load_leaf_at<T, VEC>(cx, soff, (own | amid | v1i) != 0);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) r.mid[k] = pool4<T, VEC>(r.leaf[k], pv[k], cx.sum_mode);
    r.top = pool4<T, VEC>(r.mid, v1, cx.sum_mode);
    return sh;
}

template <typename T, int VEC>
__device__ __forceinline__ void spatial_block4(const SpatialArgs& a, const SpatialCtx& cx, int t, int I, int J, int item,
                                               float* part, float* wsums, int nwave) {
    using TC = TreeConst<4>;
    constexpr int NSTAT = TC::NSTAT;
    constexpr int NUSED = TC::NNODE + 4 * TC::NPAR;          // 85 norms + 84 dots
    const LevelDims& g = a.dims;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    const int b0y = child_start(I, g.h[1]), nby = child_count(I, g.h[1]);
    const int b0x = child_start(J, g.w[1]), nbx = child_count(J, g.w[1]);
    BlockRegs<T, VEC> r;
    Pack<T, VEC> upper[4];
    bool vb[4];
    BlockGeo all;                           // every slot carries what its statistic needs: no selects
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        all.v1[k] = true; upper[k].zero();
#pragma unroll
        for (int q = 0; q < 4; ++q) all.v2[k][q] = true;
    }
    Pack<T, VEC> unused[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) unused[m].zero();
    float* mypart = part + wave * NSTAT;
    // ---- the four block slots: own block, or block (0, 0) as the alias of a missing one -----------------------------------------
#pragma unroll 1
    for (int kb = 0; kb < 4; ++kb) {
        const int vbi = ((kb >> 1) < nby) & ((kb & 1) < nbx);
        const Block3Shape sh = block3_unit<T, VEC>(cx, vbi * (b0y + (kb >> 1)), vbi * (b0x + (kb & 1)), g.h[2], g.w[2], g.h[3], g.w[3], r);
        (void)sh;
        block_stats<T, VEC, 3, 4, false>(r, all, true, 1 + kb, 1, unused, mypart, lane, 0);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
            if (kk == kb) upper[kk] = r.top;
    }
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) vb[kb] = ((kb >> 1) < nby) && ((kb & 1) < nbx);
    const Pack<T, VEC> root = pool4<T, VEC>(upper, vb, cx.sum_mode);
    {
        float s5[5];
        s5[0] = dot_pack(root, root);
#pragma unroll
        for (int k = 0; k < 4; ++k) s5[1 + k] = dot_pack(root, upper[k]);
        const float tot = wave_reduce_many<5>(s5, lane);
        bool ok;
        const int idx = wave_reduce_slot<5>(lane, ok);
        if (ok) mypart[idx == 0 ? 0 : TC::dot_id(0, idx - 1)] = tot;
    }
    lds_barrier();
    // ---- decisions, every wave for itself: fixed-order sums into the wave's own LDS row, then 84 tests in two passes -----------
    float* ws = wsums + wave * NSTAT;
    for (int s0 = lane; s0 < NUSED; s0 += kWave) {
        float acc = 0.f;
        for (int w = 0; w < nwave; ++w) acc += part[w * NSTAT + s0];
        ws[s0] = acc;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    unsigned long long passed[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int e = lane + 64 * c;
        const int ec = e < 4 * TC::NPAR ? e : 0;
        const bool pass = e < 4 * TC::NPAR && cosine_at_least(ws[TC::NNODE + ec], ws[ec >> 2], ws[ec + 1], a.thr_lo_sq);
        passed[c] = __ballot(pass);
    }
    auto stopped = [&](int p) {            // all four slot tests of parent p passed (p may be a per-lane value)
        const unsigned long long m = p < 16 ? passed[0] : passed[1];
        return ((unsigned)(m >> (4 * (p & 15))) & 15u) == 15u;
    };
    const bool stop0 = __builtin_amdgcn_readfirstlane((int)stopped(0)) != 0;
    // ---- metadata: wave 0, lane <-> leaf slot (block kb = lane >> 4, mid k, leaf q) -----------------------------------------------
    const int HW = a.H * a.W;
    const AxisGeo ry = axis_geo<false>(b0y, g.h[2], g.h[3]), rx = axis_geo<false>(b0x, g.w[2], g.w[3]);      // first block row / column
    const int RH = ry.cnt0 + (ry.n_mid - 1) * 2 + (nby - 1) * 4, RW = rx.cnt0 + (rx.n_mid - 1) * 2 + (nbx - 1) * 4;   // (a second block is 4 leaves wide)
    if (wave == 0) {
        const int kb = lane >> 4, k = (lane >> 2) & 3, q = lane & 3;
        const int dyb = kb >> 1, dxb = kb & 1, dy = k >> 1, dx = k & 1, ey = q >> 1, ex = q & 1;
        const AxisGeo ly = axis_geo<false>(b0y + dyb, g.h[2], g.h[3]), lx = axis_geo<false>(b0x + dxb, g.w[2], g.w[3]);   // per lane: its block
        const bool mine = dyb < nby && dxb < nbx && dy < ly.n_mid && dx < lx.n_mid && ey < (dy ? 2 : ly.cnt0) && ex < (dx ? 2 : lx.cnt0);
        const int my = ly.lo + (dy ? ly.cnt0 : 0), mx = lx.lo + (dx ? lx.cnt0 : 0);        // first leaf of the lane's mid
        const int y = my + ey, x = mx + ex;
        const int leaf_row = t * HW + y * a.W + x;
        const bool sb = stopped(1 + kb), sm = stopped(5 + 4 * kb + k);
        int emit_node, y2, x2;
        bool origin;
        if (stop0) { emit_node = 0; origin = lane == 0; y2 = ry.lo + RH; x2 = rx.lo + RW; }
        else if (sb) { emit_node = 1 + kb; origin = k == 0 && q == 0; y2 = ly.lo + ly.cnt0 + (ly.n_mid - 1) * 2; x2 = lx.lo + lx.cnt0 + (lx.n_mid - 1) * 2; }
        else if (sm) { emit_node = 5 + 4 * kb + k; origin = q == 0; y2 = my + (dy ? 2 : ly.cnt0); x2 = mx + (dx ? 2 : lx.cnt0); }
        else { emit_node = 21 + 16 * kb + 4 * k + q; origin = true; y2 = y + 1; x2 = x + 1; }
        const float n2 = ws[mine ? emit_node : 0];
        const unsigned long long om = __ballot(mine && origin), o1 = __ballot(mine && origin && y2 - y == 1 && x2 - x == 1);
        if (mine) {
            if (t == 0) a.cgeo[y * a.W + x] = (uint32_t)ry.lo | ((uint32_t)rx.lo << 8) | ((uint32_t)RW << 16) | ((uint32_t)RH << 24);
            if (origin) {
                a.meta[leaf_row] = ((uint32_t)y2 << 16) | (uint32_t)x2;
                a.inrm[leaf_row] = 1.0 / (sqrt((double)n2) + 1e-8);          // temporal stage: x / (|x| + 1e-8)
                a.lab_row[leaf_row] = leaf_row;
                a.gcnt[leaf_row] = 1;
                int* rc_list = a.rc_list + (int64_t)item * a.rc_stride;
                rc_list[1 + __popcll(om & ((1ull << lane) - 1ull))] = (y << 24) | (x << 16) | (y2 << 8) | x2;
                if (lane == 0) rc_list[0] = __popcll(om) | (__popcll(o1) << 16);       // slot (0, 0, 0) always exists and is an origin
            } else {
                a.meta[leaf_row] = 0u; a.lab_row[leaf_row] = -1; a.gcnt[leaf_row] = 0;
            }
        }
        if (tid == 0 && I == 0 && J == 0) a.frame_cnt[t] = 0;            // consumed (atomically) by the label stage
    }
    if (item == 0) {                                         // the counters of the later kernels
        if (tid < STTM_CNT_SLOTS) a.counts[tid] = 0;
        if (tid < 8) a.bar[tid] = 0;
        const int R = g.h[0] * g.w[0];
        for (int i = tid; i < R; i += blockDim.x) a.col_arrive[i] = 0;
    }
    // ---- features of the emitted pooled nodes (1x1 nodes of a dense input stay in x) -----------------------------------------------
    if (stop0) {
        if (cx.active && (RH * RW > 1 || !a.leaves_in_x))
            store_pack<T, VEC>(a.S, ((int64_t)t * HW + (int64_t)ry.lo * a.W + rx.lo) * a.C + cx.c0, root);
        return;
    }
#pragma unroll 1
    for (int kb = 0; kb < 4; ++kb) {
        if (!(((kb >> 1) < nby) && ((kb & 1) < nbx))) continue;
        const int bi = b0y + (kb >> 1), bj = b0x + (kb & 1);
        const bool sbk = __builtin_amdgcn_readfirstlane((int)stopped(1 + kb)) != 0;
        if (sbk) {
            const AxisGeo ly = axis_geo<false>(bi, g.h[2], g.h[3]), lx = axis_geo<false>(bj, g.w[2], g.w[3]);
            const int bh = ly.cnt0 + (ly.n_mid - 1) * 2, bw = lx.cnt0 + (lx.n_mid - 1) * 2;
            Pack<T, VEC> top;
            top.zero();
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                if (kk == kb) top = upper[kk];
            if (cx.active && (bh * bw > 1 || !a.leaves_in_x))
                store_pack<T, VEC>(a.S, ((int64_t)t * HW + (int64_t)ly.lo * a.W + lx.lo) * a.C + cx.c0, top);
            continue;
        }
        // something inside the block is emitted: mids that stopped must be stored (and, for a strided input, the leaves)
        const unsigned mids = (unsigned)__builtin_amdgcn_readfirstlane((int)((stopped(5 + 4 * kb) ? 1u : 0u) | (stopped(6 + 4 * kb) ? 2u : 0u) |
                                                                              (stopped(7 + 4 * kb) ? 4u : 0u) | (stopped(8 + 4 * kb) ? 8u : 0u)));
        if (mids == 0u && a.leaves_in_x) continue;
        const Block3Shape sh = block3_unit<T, VEC>(cx, bi, bj, g.h[2], g.w[2], g.h[3], g.w[3], r);      // re-read (L2-resident) + re-pool
        if (!cx.active) continue;
        const int64_t row0 = (int64_t)t * HW + (int64_t)sh.gy.lo * a.W + sh.gx.lo;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!((sh.v1m >> k) & 1u)) continue;
            const int dy = k >> 1, dx = k & 1;
            const int mh = dy ? 2 : sh.gy.cnt0, mw = dx ? 2 : sh.gx.cnt0;
            const int64_t rowk = row0 + (int64_t)(dy ? sh.gy.cnt0 : 0) * a.W + (dx ? sh.gx.cnt0 : 0);
            if ((mids >> k) & 1u) {
                if (mh * mw > 1 || !a.leaves_in_x) store_pack<T, VEC>(a.S, rowk * a.C + cx.c0, r.mid[k]);
            } else if (!a.leaves_in_x) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if ((q >> 1) < mh && (q & 1) < mw)
                        store_pack<T, VEC>(a.S, (rowk + (int64_t)(q >> 1) * a.W + (q & 1)) * a.C + cx.c0, r.leaf[k][q]);
            }
        }
    }
}

template <typename T, int VEC, int BL, int UL, int MAXNT, bool PERHEAD>
__global__ void __launch_bounds__(MAXNT, (PERHEAD || VEC * TypeInfo<T>::bytes > 16 || UL >= 3) ? 2 : 4) k_spatial(const SpatialArgs a0, const BatchPtrs bp) {
    SpatialArgs a = a0;                 // per-video pointers: a register copy (every index into a.dims is a compile-time constant)
    rebase(a, bp, blockIdx.y);
    constexpr int D = BL + UL;
    using TC = TreeConst<D>;
    constexpr int NSTAT = TC::NSTAT;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int nwave = blockDim.x / kWave;
    double* inrm_l = reinterpret_cast<double*>(smem_raw);         // [NNODE] 1 / (|node| + 1e-8)
    float* part = reinterpret_cast<float*>(inrm_l + TC::NNODE);   // [nwave][NSTAT]
    float* stat = part + nwave * NSTAT;                           // [NSTAT]
    int* stop = reinterpret_cast<int*>(stat + NSTAT);             // [NPAR] (>= 1)
    int* orow = stop + (TC::NPAR > 0 ? TC::NPAR : 1);             // [NNODE]
    int* lcount = orow + TC::NNODE;                               // [1] (+1 pad)

    STTM_K1_TICK(0);
    const LevelDims& g = a.dims;
    const int R = g.h[0] * g.w[0];
    // Block -> (frame, root cell): blocks are dealt to the XCDs round-robin (block b runs on XCD b % 8 -- observed, not promised; this is
    // for speed only), so all root cells of ONE frame go to ONE XCD: the alias rows of a frame (the leaves of cell (0, 0) of the odd
    // levels, read by every root cell that owns the lone first row / column: 7 of 16 on a 14 x 14 grid) are then fetched into that XCD's
    // L2 once instead of once per XCD (8 % of the kernel's fabric reads on the headline; the K1-shaped probe measured this mapping at
    // 19.0 against 19.8 us, profiles/r05a_k1_probe_rocprofv3.md).  The grid is rounded up to whole groups of 8 frames.
    const int xcd_slot = blockIdx.x & 7, per_xcd = blockIdx.x >> 3;
    const int t = (per_xcd / R) * 8 + xcd_slot;
    const int rcell = per_xcd % R;
    if (t >= a.T) return;
    const int wg = t * R + rcell;
#ifdef STTM_DEV
    if (a.dev.k1_span && threadIdx.x == 0) a.dev.k1_span[2 * wg] = wall_clock64();
#endif
    const int I = rcell / g.w[0], J = rcell % g.w[0];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;

    // 3-level trees (every run_vidqa.sh preset) take the one-shape body above: interior root cells -- every child and grandchild
    // exists, a workgroup-uniform fact -- its constant-shape instantiation, the cells that own the lone first row / column of an
    // odd level the one with (uniform) validity flags.  The general body below is for every other depth and for the per-head
    // cosine; these instantiations carry it only in the development build, where k1_var = 1 selects it (A/B).
    constexpr bool kOneShape = BL == 3 && UL <= 1 && !PERHEAD;
#ifdef STTM_DEV
    constexpr bool kGeneralToo = true;
#else
    constexpr bool kGeneralToo = false;
#endif
    if constexpr (kOneShape) {
        if (!kGeneralToo || a.k1_var != 1) {
            SpatialCtx cxi;
            spatial_ctx_init<T>(cxi, a, t, tid, VEC);
            if constexpr (UL == 0) {
                const bool interior = !(I == 0 && ((g.h[1] | g.h[2]) & 1)) && !(J == 0 && ((g.w[1] | g.w[2]) & 1));
                if (interior) spatial_block3<T, VEC, true>(a, cxi, t, I, J, wg, part, nwave);
                else spatial_block3<T, VEC, false>(a, cxi, t, I, J, wg, part, nwave);
            } else {
                spatial_block4<T, VEC>(a, cxi, t, I, J, wg, part, part + nwave * NSTAT, nwave);      // (second table: per-wave sums)
            }
            STTM_K1_TICK(4);
            STTM_K1_END();
            return;
        }
    }
    if constexpr (!kOneShape || kGeneralToo) {
    SpatialCtx cx;
    spatial_ctx_init<T>(cx, a, t, tid, VEC);

    // ---- phase 0: issue the loads of the first block, then clear LDS while they fly ------------------
    BlockGeo bg;
    BlockRegs<T, VEC> regs;
    Pack<T, VEC> alias[D];
    Pack<T, VEC> upper[4];   // UL == 1: the 4 block tops ; UL == 2: the 4 level-1 cells
    Pack<T, VEC> root;
    (void)upper;

    // A root cell that IS one register block (UL == 0: the 3-level trees of every run_vidqa.sh preset): its leaf rows are
    // requested before anything else.  Round 3: the LDS clearing, the alias cells (loads + pooling: a whole memory round trip for
    // the 7 of 16 root cells that own row 0 or column 0 of an odd level), a barrier and the alias norms used to run BEFORE the
    // first leaf load was issued -- ~870 instructions and, with aliases, a dependent round trip at the head of every workgroup.
    if constexpr (UL == 0) {
        block_geometry<BL>(g, 0, I, J, true, bg);
        load_block<T, VEC, BL>(cx, t, I, J, true, bg, regs);
    }
    for (int s = tid; s < nwave * NSTAT; s += blockDim.x) part[s] = 0.f;
    for (int s = tid; s < TC::NNODE; s += blockDim.x) orow[s] = -1;
    for (int s = tid; s < TC::NPAR; s += blockDim.x) stop[s] = 1;
    if (tid == 0) { lcount[0] = 0; lcount[1] = 0; }

    // alias features: cell (0,0) of level m is needed when some parent of level m-1 inside this root cell
    // has an invalid slot: level m has an odd height and we own row 0, or an odd width and we own col 0.
    bool need_alias[D];
#pragma unroll
    for (int m = 0; m < D; ++m) {
        need_alias[m] = m >= 1 && (((g.h[m] & 1) && I == 0) || ((g.w[m] & 1) && J == 0));
        alias[m].zero();
    }
    if constexpr (D >= 2) if (need_alias[D - 1]) alias[D - 1] = AliasPool<T, VEC, 0>::run(cx, g, t, D - 1, 0, 0);
    if constexpr (D >= 3) if (need_alias[D - 2]) alias[D - 2] = AliasPool<T, VEC, 1>::run(cx, g, t, D - 2, 0, 0);
    if constexpr (D >= 4) if (need_alias[D - 3]) alias[D - 3] = AliasPool<T, VEC, 2>::run(cx, g, t, D - 3, 0, 0);
    if constexpr (D >= 5) if (need_alias[D - 4]) alias[D - 4] = AliasPool<T, VEC, 3>::run(cx, g, t, D - 4, 0, 0);
    if constexpr (D >= 6) if (need_alias[D - 5]) alias[D - 5] = AliasPool<T, VEC, 4>::run(cx, g, t, D - 5, 0, 0);
    lds_barrier();     // LDS cleared (the alias loads, if any, stay in flight)

    float* mypart = part + wave * NSTAT;
    // alias norms
#pragma unroll
    for (int m = 1; m < D; ++m) {
        if (need_alias[m]) {
            const float tot = wave_sum(dot_pack(alias[m], alias[m]));
            if (lane == 0) mypart[TC::alias_id(m)] = tot;
        }
    }

    // ---- phase 1: pyramid + statistics ---------------------------------------------------------------
    if constexpr (UL == 0) {
        pool_block<T, VEC, BL>(cx, true, bg, regs);
        STTM_K1_TICK(1);
#ifdef STTM_DEV
        if (a.dev.k1_mode == 2) {               // ablation: loads + pooling only (one store keeps them alive)
            if (cx.active) store_pack<T, VEC>(a.S, (int64_t)wg * a.C + cx.c0, regs.top);
            return;
        }
#endif
        block_stats<T, VEC, BL, D, PERHEAD>(regs, bg, true, 0, 0, alias, mypart, lane, a.head_lanes);
        root = regs.top;
    } else if constexpr (UL == 1) {
        const CellGeo c0 = cell_children(g, 0, I, J);
        bool v0[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v0[k] = (k >> 1) < c0.rc && (k & 1) < c0.cc;
            const int bi = v0[k] ? c0.rs + (k >> 1) : 0, bj = v0[k] ? c0.cs + (k & 1) : 0;
            if (v0[k]) {
                block_geometry<BL>(g, 1, bi, bj, true, bg);
                load_and_pool_block<T, VEC, BL>(cx, t, bi, bj, true, bg, regs);
                block_stats<T, VEC, BL, D, PERHEAD>(regs, bg, true, 1 + k, 1, alias, mypart, lane, a.head_lanes);
                upper[k] = regs.top;
            } else {
                upper[k].zero();
            }
        }
        root = pool4<T, VEC>(upper, v0, cx.sum_mode);
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
    } else if constexpr (UL >= 3) {
        root = upper_cell<T, VEC, BL, D, UL, PERHEAD>(cx, g, t, 0, I, J, 0, alias, mypart, lane, a.head_lanes, regs, bg);
    } else {
        const CellGeo c0 = cell_children(g, 0, I, J);
        bool v0[4];
#pragma unroll
        for (int k0 = 0; k0 < 4; ++k0) {
            v0[k0] = (k0 >> 1) < c0.rc && (k0 & 1) < c0.cc;
            upper[k0].zero();
            if (v0[k0]) {
                const int ui = c0.rs + (k0 >> 1), uj = c0.cs + (k0 & 1);
                const CellGeo c1 = cell_children(g, 1, ui, uj);
                Pack<T, VEC> bt[4];
                bool v1[4];
#pragma unroll
                for (int k1 = 0; k1 < 4; ++k1) {
                    v1[k1] = (k1 >> 1) < c1.rc && (k1 & 1) < c1.cc;
                    bt[k1].zero();
                    if (v1[k1]) {
                        const int bi = c1.rs + (k1 >> 1), bj = c1.cs + (k1 & 1);
                        block_geometry<BL>(g, 2, bi, bj, true, bg);
                        load_and_pool_block<T, VEC, BL>(cx, t, bi, bj, true, bg, regs);
                        block_stats<T, VEC, BL, D, PERHEAD>(regs, bg, true, 4 * (1 + k0) + 1 + k1, 2, alias, mypart, lane, a.head_lanes);
                        bt[k1] = regs.top;
                    }
                }
                upper[k0] = pool4<T, VEC>(bt, v1, cx.sum_mode);
                if constexpr (PERHEAD) {
                    float s[4];
                    head_parent_ratios<T, VEC>(upper[k0], bt, v1, alias[2], a.head_lanes, lane, s);
                    const float tot = wave_reduce_many<4>(s, lane);
                    bool ok;
                    const int idx = wave_reduce_slot<4>(lane, ok);
                    if (ok) mypart[TC::dot_id(1 + k0, idx)] = tot;
                } else {
                    float s[5];
                    s[0] = dot_pack(upper[k0], upper[k0]);
#pragma unroll
                    for (int k1 = 0; k1 < 4; ++k1) s[1 + k1] = v1[k1] ? dot_pack(upper[k0], bt[k1]) : dot_pack(upper[k0], alias[2]);
                    const float tot = wave_reduce_many<5>(s, lane);
                    bool ok;
                    const int idx = wave_reduce_slot<5>(lane, ok);
                    if (ok) mypart[idx == 0 ? (1 + k0) : TC::dot_id(1 + k0, idx - 1)] = tot;
                }
            }
        }
        root = pool4<T, VEC>(upper, v0, cx.sum_mode);
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
    __syncthreads();
    STTM_K1_TICK(2);

#ifdef STTM_DEV
    if (a.dev.k1_mode == 1) return;
#endif
    decide_and_emit<D, PERHEAD>(a, t, I, J, wg, part, stat, stop, orow, lcount, inrm_l, nwave);
    STTM_K1_TICK(3);

    // ---- phase 5: store the emitted features ----------------------------------------------------------------
    if constexpr (UL == 0) {
        block_store<T, VEC, BL>(regs, 0, orow, a.S, a.C, cx, a.leaves_in_x != 0);
    } else if constexpr (UL == 1) {
        if (cx.active && orow[0] >= 0) store_pack<T, VEC>(a.S, (int64_t)orow[0] * a.C + cx.c0, root);
        if (!stop[0]) {
            const CellGeo c0 = cell_children(g, 0, I, J);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool v = (k >> 1) < c0.rc && (k & 1) < c0.cc;
                if (!v) continue;
                const int tn = 1 + k;
                if (stop[tn]) {      // the block top itself is the emitted node: still in `upper`
                    if (cx.active && orow[tn] >= 0) store_pack<T, VEC>(a.S, (int64_t)orow[tn] * a.C + cx.c0, upper[k]);
                } else {             // something below the top is emitted: re-read the block (L2-resident)
                    const int bi = c0.rs + (k >> 1), bj = c0.cs + (k & 1);
                    block_geometry<BL>(g, 1, bi, bj, true, bg);
                    load_and_pool_block<T, VEC, BL>(cx, t, bi, bj, true, bg, regs);
                    block_store<T, VEC, BL>(regs, tn, orow, a.S, a.C, cx, a.leaves_in_x != 0);
                }
            }
        }
    } else if constexpr (UL >= 3) {
        if (cx.active && orow[0] >= 0) store_pack<T, VEC>(a.S, (int64_t)orow[0] * a.C + cx.c0, root);
        if (!stop[0]) {
            const CellGeo c0 = cell_children(g, 0, I, J);
#pragma unroll 1
            for (int k = 0; k < 4; ++k) {
                if ((k >> 1) < c0.rc && (k & 1) < c0.cc)
                    store_cell<T, VEC, BL, UL - 1>(cx, g, t, 1, c0.rs + (k >> 1), c0.cs + (k & 1), 1 + k, stop, orow, a.S, a.C,
                                                   a.leaves_in_x != 0, regs, bg);
            }
        }
    } else {
        if (cx.active && orow[0] >= 0) store_pack<T, VEC>(a.S, (int64_t)orow[0] * a.C + cx.c0, root);
        if (!stop[0]) {
            const CellGeo c0 = cell_children(g, 0, I, J);
#pragma unroll
            for (int k0 = 0; k0 < 4; ++k0) {
                const bool v0 = (k0 >> 1) < c0.rc && (k0 & 1) < c0.cc;
                if (!v0) continue;
                const int un = 1 + k0;
                if (stop[un]) {
                    if (cx.active && orow[un] >= 0) store_pack<T, VEC>(a.S, (int64_t)orow[un] * a.C + cx.c0, upper[k0]);
                    continue;
                }
                const int ui = c0.rs + (k0 >> 1), uj = c0.cs + (k0 & 1);
                const CellGeo c1 = cell_children(g, 1, ui, uj);
#pragma unroll
                for (int k1 = 0; k1 < 4; ++k1) {
                    const bool v1 = (k1 >> 1) < c1.rc && (k1 & 1) < c1.cc;
                    if (!v1) continue;
                    const int bi = c1.rs + (k1 >> 1), bj = c1.cs + (k1 & 1);
                    block_geometry<BL>(g, 2, bi, bj, true, bg);
                    load_and_pool_block<T, VEC, BL>(cx, t, bi, bj, true, bg, regs);
                    block_store<T, VEC, BL>(regs, 4 * un + 1 + k1, orow, a.S, a.C, cx, a.leaves_in_x != 0);
                }
            }
        }
    }
    STTM_K1_TICK(4);
    STTM_K1_END();
    }   // general body
}


// ---------------------------------------------------------------------------------------------------
// Deep trees over several workgroups (round 4).  A root cell of a 5- / 6-level tree covers up to 16 x 16 / 32 x 32 leaves, and one
// workgroup per (frame, root cell) -- the general body above -- leaves most of the chip idle (36 x 64 tokens at root_level 0: four
// workgroups per frame).  The split form runs the tree in two launches:
//   pass A  k_spatial_blocks: one workgroup per (frame, 3-level block) -- the one-shape body of the 3-level trees on the three
//           finest levels, as if every level above had split; it also writes the block's pooled top into `tops[t][bi][bj]`;
//   pass B  k_spatial_upper: one workgroup per (frame, root cell) builds the UL upper levels from the tops (a (UL+1)-level tree
//           whose leaves are the block tops: 4 / 16 / 64 rows instead of 64 / 256 / 1024 leaf rows), runs their (parent, slot)
//           tests top-down (quadtree_builder.py:41-74: a node is emitted when every ancestor split and its own four tests pass),
//           and then walks the root cell's leaf positions once: a position under a stopped upper node takes that node's metadata
//           (its origin) or is cleared (everything else under it, overriding pass A); a position whose upper ancestors all split
//           keeps what pass A wrote.  The same walk builds the root cell's node list, the geometry table and the counters.
// The decisions are the same numbers as in the one-workgroup form: tops and upper cells are pooled level by level in the input
// dtype with pool4, the alias of an invalid slot at level m (quirk Q1) is cell (t, 0, 0) of that level pooled from the tops.
// ---------------------------------------------------------------------------------------------------
template <typename T, int VEC, int MAXNT>
__global__ void __launch_bounds__(MAXNT, (VEC * TypeInfo<T>::bytes > 16) ? 2 : 4) k_spatial_blocks(const SpatialArgs a0, const BatchPtrs bp, void* tops0) {
    SpatialArgs a = a0;                 // a.dims: the block level and the two levels below it
    rebase(a, bp, blockIdx.y);
    void* tops = tops0;
    if (blockIdx.y) shift_ptr(tops, (size_t)blockIdx.y * bp.ws_stride);
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* part = reinterpret_cast<float*>(smem_raw);             // [nwave][NSTAT of a 3-level tree]
    const LevelDims& g = a.dims;
    const int RB = g.h[0] * g.w[0];
    const int t = blockIdx.x / RB, b = blockIdx.x % RB;
    const int I = b / g.w[0], J = b % g.w[0];
    SpatialCtx cx;
    spatial_ctx_init<T>(cx, a, t, threadIdx.x, VEC);
    const int nwave = blockDim.x / kWave;
    const bool interior = !(I == 0 && ((g.h[1] | g.h[2]) & 1)) && !(J == 0 && ((g.w[1] | g.w[2]) & 1));
    if (interior) spatial_block3<T, VEC, true, true>(a, cx, t, I, J, blockIdx.x, part, nwave, tops);
    else spatial_block3<T, VEC, false, true>(a, cx, t, I, J, blockIdx.x, part, nwave, tops);
}

// pooled feature of cell (i, j) of level UL - UREM, from the block tops (UREM = levels between the cell and the tops)
template <typename T, int VEC, int UL, int UREM>
__device__ __forceinline__ Pack<T, VEC> tops_cell(const void* tops, const SpatialArgs& a, const SpatialCtx& cx, int t, int i, int j) {
    const LevelDims& g = a.dims;
    if constexpr (UREM == 0) {
        Pack<T, VEC> p;
        p.zero();
        if (cx.active) p = load_pack<T, VEC>(tops, ((int64_t)(t * g.h[UL] + i) * g.w[UL] + j) * a.C + cx.c0);
        return p;
    } else {
        const CellGeo c = cell_children(g, UL - UREM, i, j);
        Pack<T, VEC> ch[4];
        bool v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { ch[k].zero(); v[k] = false; }
        if constexpr (UREM == 1) {           // the four tops of a lowest upper cell: requested together
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = (k >> 1) < c.rc && (k & 1) < c.cc;
                if (v[k]) ch[k] = tops_cell<T, VEC, UL, 0>(tops, a, cx, t, c.rs + (k >> 1), c.cs + (k & 1));
            }
        } else {
#pragma unroll 1
            for (int k = 0; k < 4; ++k) {
                if ((k >> 1) < c.rc && (k & 1) < c.cc) {
                    const Pack<T, VEC> r = tops_cell<T, VEC, UL, UREM - 1>(tops, a, cx, t, c.rs + (k >> 1), c.cs + (k & 1));
                    keep_child<T, VEC>(ch, v, k, r, true);
                }
            }
        }
        return pool4<T, VEC>(ch, v, cx.sum_mode);
    }
}
// the same with the statistics of the cell and of everything below it accumulated into this wave's partial table (tree node tn of
// the (UL+1)-level tree over the tops): |cell|^2 for every cell, cell . child (or . alias of the child level) for every parent.
// Every upper cell's feature is also left in `uf` (this root cell's [upper node][C] table): the ones that turn out to be emitted
// are copied to S after the decisions (rebuilding them from the tops was 3-10 us of dependent loads per workgroup).
template <typename T, int VEC, int UL, int UREM>
__device__ __forceinline__ Pack<T, VEC> tops_cell_stats(const void* tops, const SpatialArgs& a, const SpatialCtx& cx, int t, int i, int j, int tn,
                                                        const Pack<T, VEC> (&alias)[UL + 1], float* mypart, int lane, void* uf) {
    using TC = TreeConst<UL + 1>;
    if constexpr (UREM == 0) {
        const Pack<T, VEC> p = tops_cell<T, VEC, UL, 0>(tops, a, cx, t, i, j);
        const float tot = wave_sum(dot_pack(p, p));
        if (lane == 0) mypart[tn] = tot;
        return p;
    } else if constexpr (UREM == 1) {
        // a lowest upper cell: its four tops are requested together (one memory round trip per cell instead of four -- with one
        // workgroup per root cell the 64 tops of a 6-level tree were 64 dependent round trips, 85 of the pass's 125 us) and the
        // nine sums -- |cell|^2, cell . top_k (or . alias), |top_k|^2 -- share one butterfly
        const CellGeo c = cell_children(a.dims, UL - 1, i, j);
        Pack<T, VEC> ch[4];
        bool v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = (k >> 1) < c.rc && (k & 1) < c.cc;
            ch[k].zero();
            if (v[k]) ch[k] = tops_cell<T, VEC, UL, 0>(tops, a, cx, t, c.rs + (k >> 1), c.cs + (k & 1));
        }
        const Pack<T, VEC> me = pool4<T, VEC>(ch, v, cx.sum_mode);
        float s[9];
        s[0] = dot_pack(me, me);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s[1 + k] = v[k] ? dot_pack(me, ch[k]) : dot_pack(me, alias[UL]);
            s[5 + k] = dot_pack(ch[k], ch[k]);
        }
        const float tot = wave_reduce_many<9, 2>(s, lane);
        bool ok;
        const int idx = wave_reduce_slot<9>(lane, ok);
        if (ok) mypart[idx == 0 ? tn : (idx < 5 ? TC::dot_id(tn, idx - 1) : 4 * tn + 1 + (idx - 5))] = tot;
        if constexpr (UL > 1)               // (one upper level: the root stays in the caller's registers)
            if (cx.active) store_pack<T, VEC>(uf, (int64_t)tn * a.C + cx.c0, me);
        return me;
    } else if constexpr (UREM == 2) {
        // two levels above the tops: the (up to) sixteen tops under this cell are requested together -- a 3-level block whose
        // leaves are block tops --, then the four lowest upper cells and this cell are pooled and reduced from registers
        const LevelDims& g = a.dims;
        const CellGeo c = cell_children(g, UL - 2, i, j);
        Pack<T, VEC> tp[4][4], mid[4];
        bool v1[4], v2[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v1[k] = (k >> 1) < c.rc && (k & 1) < c.cc;
            const CellGeo m = cell_children(g, UL - 1, v1[k] ? c.rs + (k >> 1) : 0, v1[k] ? c.cs + (k & 1) : 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                v2[k][q] = v1[k] && (q >> 1) < m.rc && (q & 1) < m.cc;
                tp[k][q].zero();
                if (v2[k][q]) tp[k][q] = tops_cell<T, VEC, UL, 0>(tops, a, cx, t, m.rs + (q >> 1), m.cs + (q & 1));
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mid[k].zero();
            if (!v1[k]) continue;                    // (uniform)
            mid[k] = pool4<T, VEC>(tp[k], v2[k], cx.sum_mode);
            const int tk = 4 * tn + 1 + k;
            if (cx.active) store_pack<T, VEC>(uf, (int64_t)tk * a.C + cx.c0, mid[k]);
            float s[9];
            s[0] = dot_pack(mid[k], mid[k]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                s[1 + q] = v2[k][q] ? dot_pack(mid[k], tp[k][q]) : dot_pack(mid[k], alias[UL]);
                s[5 + q] = dot_pack(tp[k][q], tp[k][q]);
            }
            const float tot = wave_reduce_many<9, 2>(s, lane);
            bool ok;
            const int idx = wave_reduce_slot<9>(lane, ok);
            if (ok) mypart[idx == 0 ? tk : (idx < 5 ? TC::dot_id(tk, idx - 1) : 4 * tk + 1 + (idx - 5))] = tot;
        }
        const Pack<T, VEC> me = pool4<T, VEC>(mid, v1, cx.sum_mode);
        if (cx.active) store_pack<T, VEC>(uf, (int64_t)tn * a.C + cx.c0, me);
        float s[5];
        s[0] = dot_pack(me, me);
#pragma unroll
        for (int k = 0; k < 4; ++k) s[1 + k] = v1[k] ? dot_pack(me, mid[k]) : dot_pack(me, alias[UL - 1]);
        const float tot = wave_reduce_many<5, 2>(s, lane);
        bool ok;
        const int idx = wave_reduce_slot<5>(lane, ok);
        if (ok) mypart[idx == 0 ? tn : TC::dot_id(tn, idx - 1)] = tot;
        return me;
    } else {
        const CellGeo c = cell_children(a.dims, UL - UREM, i, j);
        Pack<T, VEC> ch[4];
        bool v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { ch[k].zero(); v[k] = false; }
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            if ((k >> 1) < c.rc && (k & 1) < c.cc) {
                const Pack<T, VEC> r = tops_cell_stats<T, VEC, UL, UREM - 1>(tops, a, cx, t, c.rs + (k >> 1), c.cs + (k & 1), 4 * tn + 1 + k,
                                                                             alias, mypart, lane, uf);
                keep_child<T, VEC>(ch, v, k, r, true);
            }
        }
        const Pack<T, VEC> me = pool4<T, VEC>(ch, v, cx.sum_mode);
        if (cx.active) store_pack<T, VEC>(uf, (int64_t)tn * a.C + cx.c0, me);
        float s[5];
        s[0] = dot_pack(me, me);
#pragma unroll
        for (int k = 0; k < 4; ++k) s[1 + k] = v[k] ? dot_pack(me, ch[k]) : dot_pack(me, alias[UL - UREM + 1]);
        const float tot = wave_reduce_many<5, 2>(s, lane);
        bool ok;
        const int idx = wave_reduce_slot<5>(lane, ok);
        if (ok) mypart[idx == 0 ? tn : TC::dot_id(tn, idx - 1)] = tot;
        return me;
    }
}
template <typename T, int VEC, int UL, int MAXNT>
__global__ void __launch_bounds__(MAXNT) k_spatial_upper(const SpatialArgs a0, const BatchPtrs bp, const void* tops0, void* ufeat0) {
    SpatialArgs a = a0;
    rebase(a, bp, blockIdx.y);
    const void* tops = tops0;
    void* uf = ufeat0;                  // [T * R][upper nodes][C]: the pooled features of the upper cells
    if (blockIdx.y) { shift_ptr(tops, (size_t)blockIdx.y * bp.ws_stride); shift_ptr(uf, (size_t)blockIdx.y * bp.ws_stride); }
    constexpr int D = UL + 3;           // levels of the whole tree
    constexpr int DU = UL + 1;          // levels of the tree over the tops
    using TC = TreeConst<DU>;
    constexpr int NSTAT = TC::NSTAT, NPAR = TC::NPAR;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int nwave = blockDim.x / kWave;
    double* inrm_l = reinterpret_cast<double*>(smem_raw);         // [NPAR] 1 / (|upper node| + 1e-8)
    float* part = reinterpret_cast<float*>(inrm_l + NPAR);        // [nwave][NSTAT]
    float* stat = part + nwave * NSTAT;                           // [NSTAT]
    int* stop = reinterpret_cast<int*>(stat + NSTAT);             // [NPAR]
    int* orow = stop + NPAR;                                      // [NPAR]
    int* lcount = orow + NPAR;                                    // [2]

    const LevelDims& g = a.dims;
    const int R = g.h[0] * g.w[0];
    const int t = blockIdx.x / R, rcell = blockIdx.x % R;
    const int I = rcell / g.w[0], J = rcell % g.w[0];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int HW = a.H * a.W;
    SpatialCtx cx;
    spatial_ctx_init<T>(cx, a, t, tid, VEC);

    STTM_K1_TICK(8);
    // what pass A left at this thread's leaf positions: requested now, used after the decisions
    constexpr int NLEAF = pow4(D - 1);
    constexpr int KQ = 4;
    uint32_t pm[KQ];
#pragma unroll
    for (int k = 0; k < KQ; ++k) {
        pm[k] = 0u;
        const int q = tid + k * (int)blockDim.x;
        if (q < NLEAF) {
            const NodeLoc L = locate_static<D - 1>(g, I, J, q);
            if (L.valid) pm[k] = a.meta[t * HW + L.i * a.W + L.j];
        }
    }
    for (int s = tid; s < nwave * NSTAT; s += blockDim.x) part[s] = 0.f;
    for (int s = tid; s < NPAR; s += blockDim.x) { stop[s] = 1; orow[s] = -1; }
    if (tid == 0) { lcount[0] = 0; lcount[1] = 0; }
    // aliases: cell (0, 0) of level m is what an invalid child slot of a level m-1 parent is compared with -- needed when this
    // root cell owns row 0 of a level with an odd height or column 0 of one with an odd width
    Pack<T, VEC> alias[DU];
    bool need_alias[DU];
#pragma unroll
    for (int m = 0; m < DU; ++m) {
        need_alias[m] = m >= 1 && (((g.h[m] & 1) && I == 0) || ((g.w[m] & 1) && J == 0));
        alias[m].zero();
    }
    if constexpr (UL >= 1) if (need_alias[UL]) alias[UL] = tops_cell<T, VEC, UL, 0>(tops, a, cx, t, 0, 0);
    if constexpr (UL >= 2) if (need_alias[UL - 1]) alias[UL - 1] = tops_cell<T, VEC, UL, 1>(tops, a, cx, t, 0, 0);
    if constexpr (UL >= 3) if (need_alias[UL - 2]) alias[UL - 2] = tops_cell<T, VEC, UL, 2>(tops, a, cx, t, 0, 0);
    lds_barrier();
    float* mypart = part + wave * NSTAT;
#pragma unroll
    for (int m = 1; m < DU; ++m) {
        if (need_alias[m]) {
            const float tot = wave_sum(dot_pack(alias[m], alias[m]));
            if (lane == 0) mypart[TC::alias_id(m)] = tot;
        }
    }
    STTM_K1_TICK(9);
    uf = reinterpret_cast<char*>(uf) + (size_t)blockIdx.x * NPAR * a.C * TypeInfo<T>::bytes;
    const Pack<T, VEC> rootp = tops_cell_stats<T, VEC, UL, UL>(tops, a, cx, t, I, J, 0, alias, mypart, lane, uf);
    __syncthreads();
    STTM_K1_TICK(10);
    // cross-wave sums in a fixed order, then every (parent, slot) test of the upper levels and the upper nodes' inverse norms
    for (int s2 = tid; s2 < NSTAT; s2 += blockDim.x) {
        float acc = 0.f;
        for (int w = 0; w < nwave; ++w) acc += part[w * NSTAT + s2];
        stat[s2] = acc;
    }
    lds_barrier();
    for (int e = tid; e < 4 * NPAR; e += blockDim.x) {
        const int p = e >> 2, k = e & 3;
        if (p < depth_base(1)) parent_slot_test<DU, 0, false>(a, I, J, p, k, stat, stop);
        else if constexpr (UL >= 2) {
            if (p < depth_base(2)) parent_slot_test<DU, 1, false>(a, I, J, p - depth_base(1), k, stat, stop);
            else if constexpr (UL >= 3) parent_slot_test<DU, 2, false>(a, I, J, p - depth_base(2), k, stat, stop);
        }
    }
    for (int n = tid; n < NPAR; n += blockDim.x) inrm_l[n] = 1.0 / (sqrt((double)stat[n]) + 1e-8);
    lds_barrier();
    STTM_K1_TICK(11);
    // ---- one thread per leaf position of the root cell ------------------------------------------------------------------------
    // (what pass A left at the position -- `meta`: non-zero exactly where a node starts -- was requested at the top of the kernel;
    // list positions come from one ballot per wave and iteration, not from one LDS atomic per node)
    int* rc_list = a.rc_list + (int64_t)blockIdx.x * a.rc_stride;
    for (int it = 0, q = tid; q < NLEAF; ++it, q += blockDim.x) {
        const NodeLoc L = locate_static<D - 1>(g, I, J, q);
        const int leaf_row = t * HW + L.i * a.W + L.j;
        if (L.valid && t == 0) {
            int lo_i = I, hi_i = I, lo_j = J, hi_j = J;
#pragma unroll
            for (int m = 0; m < D - 1; ++m) {
                lo_i = child_start(lo_i, g.h[m + 1]);
                hi_i = child_start(hi_i, g.h[m + 1]) + child_count(hi_i, g.h[m + 1]) - 1;
                lo_j = child_start(lo_j, g.w[m + 1]);
                hi_j = child_start(hi_j, g.w[m + 1]) + child_count(hi_j, g.w[m + 1]) - 1;
            }
            a.cgeo[L.i * a.W + L.j] = (uint32_t)lo_i | ((uint32_t)lo_j << 8) | ((uint32_t)(hi_j - lo_j + 1) << 16) | ((uint32_t)(hi_i - lo_i + 1) << 24);
        }
        int da = -1;
#pragma unroll
        for (int d = UL - 1; d >= 0; --d)
            if (stop[L.path[d]]) da = d;                       // the SHALLOWEST stopped upper ancestor
        bool node = false;
        int y2 = 0, x2 = 0;
        if (L.valid && da < 0) {
            // every upper ancestor split: what pass A decided inside the block stands
            uint32_t m = 0;
#pragma unroll
            for (int k = 0; k < KQ; ++k)
                if (it == k) m = pm[k];
            if (it >= KQ) m = a.meta[leaf_row];
            node = m != 0u;
            y2 = (int)(m >> 16); x2 = (int)(m & 0xffffu);
        } else if (L.valid) {
            bool origin = true;
            int emit_node = 0, hi_i = 0, hi_j = 0;
#pragma unroll
            for (int d = D - 1; d >= 0; --d) {
                if (d > da) origin = origin && (L.slot[d] == 0);
                if (d == da) { emit_node = L.path[d]; hi_i = L.pi[d]; hi_j = L.pj[d]; }
            }
            if (!origin) { a.meta[leaf_row] = 0u; a.lab_row[leaf_row] = -1; a.gcnt[leaf_row] = 0; }
            else {
#pragma unroll
                for (int m = 0; m < D - 1; ++m) {
                    if (m >= da) {
                        hi_i = child_start(hi_i, g.h[m + 1]) + child_count(hi_i, g.h[m + 1]) - 1;
                        hi_j = child_start(hi_j, g.w[m + 1]) + child_count(hi_j, g.w[m + 1]) - 1;
                    }
                }
                y2 = hi_i + 1; x2 = hi_j + 1;
                a.meta[leaf_row] = ((uint32_t)y2 << 16) | (uint32_t)x2;
                a.inrm[leaf_row] = inrm_l[emit_node];
                a.lab_row[leaf_row] = leaf_row;
                a.gcnt[leaf_row] = 1;
                orow[emit_node] = leaf_row;
                node = true;
            }
        }
        const unsigned long long nm = __ballot(node), n1 = __ballot(node && y2 - L.i == 1 && x2 - L.j == 1);
        if (nm) {                                              // (uniform)
            int base = 0;
            if (lane == 0) { base = atomicAdd(lcount, __popcll(nm)); if (n1) atomicAdd(lcount + 1, __popcll(n1)); }
            base = __shfl(base, 0, 64);
            if (node) rc_list[1 + base + __popcll(nm & ((1ull << lane) - 1ull))] = (L.i << 24) | (L.j << 16) | (y2 << 8) | x2;
        }
    }
    STTM_K1_TICK(12);
    lds_barrier();
    if (tid == 0) {
        rc_list[0] = lcount[0] | (lcount[1] << 16);          // nodes | 1x1 nodes of this (frame, root cell)
        if (I == 0 && J == 0) a.frame_cnt[t] = 0;            // consumed (atomically) by the label stage
    }
    if (blockIdx.x == 0) {                                   // the counters of the later kernels
        if (tid < STTM_CNT_SLOTS) a.counts[tid] = 0;
        if (tid < 8) a.bar[tid] = 0;
        for (int i = tid; i < R; i += blockDim.x) a.col_arrive[i] = 0;
    }
    // features of the emitted upper nodes (orow: set by the node's origin position in the walk above): uf -> S, four rows in flight
    // (every lane reads back the channels it wrote itself)
    if constexpr (UL == 1) {            // the root is the only upper node: still in registers (no table round trip: 4-level grids, config 4)
        if (cx.active && orow[0] >= 0) store_pack<T, VEC>(a.S, (int64_t)orow[0] * a.C + cx.c0, rootp);
    } else if (cx.active) {
        for (int n0 = 0; n0 < NPAR; n0 += 4) {
            Pack<T, VEC> v[4];
            int r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                r[k] = n0 + k < NPAR ? orow[n0 + k] : -1;
                if (r[k] >= 0) v[k] = load_pack<T, VEC>(uf, (int64_t)(n0 + k) * a.C + cx.c0);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (r[k] >= 0) store_pack<T, VEC>(a.S, (int64_t)r[k] * a.C + cx.c0, v[k]);
        }
    }
    STTM_K1_TICK(13);
}

// ---------------------------------------------------------------------------------------------------
// host-side dispatch
// ---------------------------------------------------------------------------------------------------
template <typename T, int VEC, int BL, int UL, bool PERHEAD>
static hipError_t launch_bl_ul(const SpatialArgs& a, const BatchPtrs& bp, int n_videos, int grid, int nt, hipStream_t stream) {
    constexpr int D = BL + UL;
    using TC = TreeConst<D>;
    const int nwave = nt / kWave;
    constexpr int kTables = (BL == 3 && UL == 1 && !PERHEAD) ? 2 : 1;      // per-wave partial sums (+ per-wave totals: the 4-level one-shape body)
    const size_t smem = sizeof(double) * TC::NNODE + sizeof(float) * ((size_t)kTables * nwave * TC::NSTAT + TC::NSTAT) +
                        sizeof(int) * ((TC::NPAR > 0 ? TC::NPAR : 1) + TC::NNODE + 4);
    const dim3 g3(grid, n_videos);
    if (nt <= 256) hipLaunchKernelGGL((k_spatial<T, VEC, BL, UL, 256, PERHEAD>), g3, dim3(nt), smem, stream, a, bp);
    else if (nt <= 512) hipLaunchKernelGGL((k_spatial<T, VEC, BL, UL, 512, PERHEAD>), g3, dim3(nt), smem, stream, a, bp);
    else hipLaunchKernelGGL((k_spatial<T, VEC, BL, UL, 1024, PERHEAD>), g3, dim3(nt), smem, stream, a, bp);
    return hipGetLastError();
}

// the split form of a deep tree: pass A over the 3-level blocks, pass B over the upper levels
template <typename T, int VEC, int UL>
static hipError_t launch_split(const SpatialArgs& a, const BatchPtrs& bp, int n_videos, int nt, hipStream_t stream, void* tops) {
    // (the table of the upper cells' features follows the block tops: api.hip, carve_all)
    void* ufeat = reinterpret_cast<char*>(tops) + split_tops_bytes(a.T, a.dims, a.C, (int)TypeInfo<T>::bytes);
    SpatialArgs ab = a;
    ab.dims = LevelDims{};
    ab.dims.n_level = 3;
    for (int l = 0; l < 3; ++l) { ab.dims.h[l] = a.dims.h[UL + l]; ab.dims.w[l] = a.dims.w[UL + l]; }
    const int nwave = nt / kWave;
    const dim3 ga(a.T * ab.dims.h[0] * ab.dims.w[0], n_videos);
    const size_t smem_a = sizeof(float) * (size_t)nwave * TreeConst<3>::NSTAT;
    constexpr bool kWide = VEC * TypeInfo<T>::bytes > 16;      // 32-byte packs: rows of at most 512 lanes (api.hip: pick_vec)
    if (nt <= 256) hipLaunchKernelGGL((k_spatial_blocks<T, VEC, 256>), ga, dim3(nt), smem_a, stream, ab, bp, tops);
    else if (nt <= 512) hipLaunchKernelGGL((k_spatial_blocks<T, VEC, 512>), ga, dim3(nt), smem_a, stream, ab, bp, tops);
    else if constexpr (!kWide) hipLaunchKernelGGL((k_spatial_blocks<T, VEC, 1024>), ga, dim3(nt), smem_a, stream, ab, bp, tops);
    else return hipErrorInvalidValue;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    using TC = TreeConst<UL + 1>;
    const dim3 gb(a.T * a.dims.h[0] * a.dims.w[0], n_videos);
    const size_t smem_b = sizeof(double) * TC::NPAR + sizeof(float) * ((size_t)nwave * TC::NSTAT + TC::NSTAT) + sizeof(int) * (2 * TC::NPAR + 2);
    if (nt <= 256) hipLaunchKernelGGL((k_spatial_upper<T, VEC, UL, 256>), gb, dim3(nt), smem_b, stream, a, bp, (const void*)tops, ufeat);
    else if constexpr (kWide) hipLaunchKernelGGL((k_spatial_upper<T, VEC, UL, 512>), gb, dim3(nt), smem_b, stream, a, bp, (const void*)tops, ufeat);
    else hipLaunchKernelGGL((k_spatial_upper<T, VEC, UL, 1024>), gb, dim3(nt), smem_b, stream, a, bp, (const void*)tops, ufeat);
    return hipGetLastError();
}

template <typename T, int VEC, bool PERHEAD>
static hipError_t launch_depth(const SpatialArgs& a, const BatchPtrs& bp, int n_videos, int grid, int nt, hipStream_t stream, void* tops) {
    if constexpr (!PERHEAD) {
        if (tops) {
            switch (a.dims.n_level) {
                case 4: return launch_split<T, VEC, 1>(a, bp, n_videos, nt, stream, tops);
                case 5: return launch_split<T, VEC, 2>(a, bp, n_videos, nt, stream, tops);
                case 6: return launch_split<T, VEC, 3>(a, bp, n_videos, nt, stream, tops);
                default: break;
            }
        }
    }
    switch (a.dims.n_level) {
        case 1: return launch_bl_ul<T, VEC, 1, 0, PERHEAD>(a, bp, n_videos, grid, nt, stream);
        case 2: return launch_bl_ul<T, VEC, 2, 0, PERHEAD>(a, bp, n_videos, grid, nt, stream);
        case 3: return launch_bl_ul<T, VEC, 3, 0, PERHEAD>(a, bp, n_videos, grid, nt, stream);
        case 4: return launch_bl_ul<T, VEC, 3, 1, PERHEAD>(a, bp, n_videos, grid, nt, stream);
        case 5: return launch_bl_ul<T, VEC, 3, 2, PERHEAD>(a, bp, n_videos, grid, nt, stream);
        case 6: return launch_bl_ul<T, VEC, 3, 3, PERHEAD>(a, bp, n_videos, grid, nt, stream);
        default: return hipErrorInvalidValue;
    }
}

// ---------------------------------------------------------------------------------------------------
// Node apply: pool ANOTHER tensor (RoPE cos / sin of the position-embedding ablation, quadtree_builder.py:75-81 and
// quadtree_spatial_merger.py:88-153) over the nodes the spatial kernel already decided, with the same pyramid
// arithmetic.  One workgroup per (frame, root cell) walks that cell's node list; every leaf is read once.
// ---------------------------------------------------------------------------------------------------
template <typename T, int VEC, int MAXNT>
__global__ void __launch_bounds__(MAXNT) k_node_apply(SpatialArgs a) {
    const LevelDims& g = a.dims;
    const int D = g.n_level;
    const int R = g.h[0] * g.w[0];
    const int t = blockIdx.x / R;
    const int* list = a.rc_list + (int64_t)blockIdx.x * a.rc_stride;
    const int n = list[0] & 0xffff;
    const int HW = a.H * a.W;
    SpatialCtx cx;
    spatial_ctx_init<T>(cx, a, t, threadIdx.x, VEC);
    for (int k = 0; k < n; ++k) {
        const unsigned b = (unsigned)list[1 + k];
        const int y1 = b >> 24, x1 = (b >> 16) & 255, y2 = (b >> 8) & 255, x2 = b & 255;
        if (a.leaves_in_x && y2 - y1 == 1 && x2 - x1 == 1) continue;       // consumers read 1x1 rows from the tensor itself
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
        Pack<T, VEC> v;
        switch (D - 1 - lvl) {
            case 0: v = AliasPool<T, VEC, 0>::run(cx, g, t, lvl, ci, cj); break;
            case 1: v = AliasPool<T, VEC, 1>::run(cx, g, t, lvl, ci, cj); break;
            case 2: v = AliasPool<T, VEC, 2>::run(cx, g, t, lvl, ci, cj); break;
            case 3: v = AliasPool<T, VEC, 3>::run(cx, g, t, lvl, ci, cj); break;
            case 4: v = AliasPool<T, VEC, 4>::run(cx, g, t, lvl, ci, cj); break;
            default: v = AliasPool<T, VEC, 5>::run(cx, g, t, lvl, ci, cj); break;       // kMaxLevels = 6: a root cell
        }
        if (cx.active) store_pack<T, VEC>(a.S, (int64_t)(t * HW + y1 * a.W + x1) * a.C + cx.c0, v);
    }
}

template <typename T>
hipError_t launch_apply_t(const SpatialArgs& a, int vec, int nt, hipStream_t stream);

// per-dtype entry point, explicitly instantiated by one translation unit per (dtype, per-head) combination
template <typename T> struct VecChoices { static constexpr int a = 4, b = 2, c = 1, wide = 8; };
template <> struct VecChoices<bf16_t> { static constexpr int a = 8, b = 4, c = 2, wide = 16; };
template <> struct VecChoices<f16_t> { static constexpr int a = 8, b = 4, c = 2, wide = 16; };

template <typename T, bool PERHEAD>
hipError_t launch_spatial_t(const SpatialArgs& a, const BatchPtrs& bp, int n_videos, int vec, int nt, hipStream_t stream, void* tops) {
    const int grid = (a.T + 7) / 8 * 8 * a.dims.h[0] * a.dims.w[0];          // k_spatial: whole groups of 8 frames (one frame per XCD)
    using V = VecChoices<T>;
    if constexpr (V::wide > 0 && !PERHEAD) {
        if (vec == V::wide) return launch_depth<T, V::wide, PERHEAD>(a, bp, n_videos, grid, nt, stream, tops);
    }
    if (vec == V::a) return launch_depth<T, V::a, PERHEAD>(a, bp, n_videos, grid, nt, stream, tops);
    if (vec == V::b) return launch_depth<T, V::b, PERHEAD>(a, bp, n_videos, grid, nt, stream, tops);
    if (vec == V::c) return launch_depth<T, V::c, PERHEAD>(a, bp, n_videos, grid, nt, stream, tops);
    return hipErrorInvalidValue;
}

template <typename T>
hipError_t launch_apply_t(const SpatialArgs& a, int vec, int nt, hipStream_t stream) {
    const int grid = a.T * a.dims.h[0] * a.dims.w[0];
    using V = VecChoices<T>;
#define STTM_LAUNCH_APPLY(VV) hipLaunchKernelGGL((k_node_apply<T, VV, 1024>), dim3(grid), dim3(nt), 0, stream, a)
    if (vec == V::a) STTM_LAUNCH_APPLY(V::a);
    else if (vec == V::b) STTM_LAUNCH_APPLY(V::b);
    else if (vec == V::c) STTM_LAUNCH_APPLY(V::c);
    else return hipErrorInvalidValue;
#undef STTM_LAUNCH_APPLY
    return hipGetLastError();
}

}  // namespace sttm
