"""Inputs and yardsticks for the DyCoke kernels off their usual test distribution: stage 1 (csrc/dycoke.hip) at every width
class of its launcher and on clips with non-finite or degenerate tokens, stage 2 (csrc/dycoke_decode.hip) at group sizes past one
sweep, on a peaked logit family with an attention sink, and on awkward layouts.  Shared by tests/test_dycoke_offdist_cpu.py,
tests/test_hip_dycoke_offdist.py and tests/golden/make_golden_dycoke.py.  Everything here is built on the CPU; nothing imports the
device library.
"""
import functools
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import dycoke_oracle as D
from sttm_amd.synth import iid_video, synth_video
from tests import _dycoke_decode_ref as R
from tests._golden import GOLDEN_DIR

DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
SHORT = {"float32": "f32", "bfloat16": "bf16", "float16": "f16"}

# ---------------------------------------------------------------------------------------------------------------------------------
# stage 1: width classes (launch_dycoke of csrc/dycoke.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
WIDTH_T, WIDTH_SIDE, WIDTH_PRUNE = 6, 7, 0.5          # three pass-1 pairs, one pass-2 pair; P = 49, k = 24

# (C, family, seed): float32.                               similarity kernel                       gather
FP32_WIDTHS = [
    (1024, "iid", 1),     # k_dycoke_sim<4>, every lane's four chunks live                          k_dycoke_gather<4>
    (1028, "synth", 2),   # k_dycoke_sim<8>, chunk 4 live on lane 0 only, 5..7 dead                 k_dycoke_gather<8>
    (2048, "iid", 3),     # k_dycoke_sim<8>, full                                                   k_dycoke_gather<8>
    (2052, "synth", 4),   # k_dycoke_sim<16>, chunk 8 live on lane 0 only                           k_dycoke_gather<16>
    (3584, "iid", 5),     # k_dycoke_sim<16>, 14 of 16 chunks (the production width)                k_dycoke_gather<16>
    (4096, "synth", 6),   # k_dycoke_sim<16>, full                                                  k_dycoke_gather<16>
    (4100, "iid", 7),     # k_dycoke_sim<0>: C % 4 == 0 but C > 4096                                k_dycoke_gather<0>
    (1026, "synth", 8),   # k_dycoke_sim<0>: C % 4 != 0                                             k_dycoke_gather<0>
    (6, "iid", 9),        # k_dycoke_sim<0>, 58 idle lanes                                          k_dycoke_gather<0>
]
# Seeds: chosen so that at most 1 of the 96 kept tokens lies within 2 ulps of a cut (tests/test_dycoke_offdist_cpu.py asserts it).
# (C, family, seed): bfloat16 and float16.                  similarity kernel                       gather on C / 2 words
LOWP_WIDTHS = [
    (512, "iid", 11),     # k_dycoke_sim16<T, true>, one trip of `c += 512`, all lanes              <4>  (256 words)
    (520, "iid", 22),     # <T, true>, second trip on lane 0 only                                   <4>  (260)
    (1024, "iid", 13),    # <T, true>, two full trips                                               <4>  (512)
    (3584, "iid", 14),    # <T, true>, seven trips (Qwen2-7B hidden size)                           <8>  (1792)
    (4104, "iid", 15),    # <T, true>, nine trips, the last on lane 0 only                          <16> (2052)
    (1022, "iid", 16),    # <T, false> (C % 8 != 0)                                                 <0>  (511 words: not % 4)
    (100, "iid", 27),     # <T, false>                                                              <0>  (50)
]
# Structured, correlated rows at 16 bits: default synth_video in float16 only (its similarities lie in [0.3, 0.9], where bfloat16 is too
# coarse for `near <= 2 %`, profiles/dycoke_offdist.md).  Seeds: the first from 50 on with `near` = 0.
LOWP_SYNTH_F16 = [
    (3584, "synth", 55),  # <f16, true>, seven trips                                                 <8>
    (520, "synth", 50),   # <f16, true>, second trip on lane 0 only                                  <4>
]
LOWP_CASES = ([(C, fam, seed, d) for d in ("bfloat16", "float16") for C, fam, seed in LOWP_WIDTHS]
              + [(C, fam, seed, "float16") for C, fam, seed in LOWP_SYNTH_F16])
# (T, C): the odd last frame (T = 7: n1 = 3, n2 = 1; T = 9: n1 = 4, n2 = 2, a whole frame 8) through k_dycoke_gather<16>
ODD_T_CASES = [(7, 2052), (9, 2052)]

# (H, W) of the P edges: float32, C = 16, T = 5 (pairs (0,1), (2,3), pass 2 (0,2); frame 4 whole)
P_EDGES = [
    (1, 1),      # P = 1: npad = 1, the sort loops never run
    (7, 9),      # P = 63: npad = 64, one pad entry, one wave of select threads
    (8, 8),      # P = 64: npad = 64, no pad entry
    (5, 13),     # P = 65: npad = 128, 63 pad entries, two waves
    (27, 27),    # P = 729: npad = 1024, 1024 threads, one element each
    (36, 36),    # P = 1296: npad = 2048, the `i += nt` loops make two trips
    (32, 64),    # P = 2048: the limit, no pad entry
]
P_TOO_MANY = (3, 683)    # P = 2049: refused before any launch


def frames_to_rows(vid):
    """[T, C, H, W] view of [T, H, W, C] memory -> the [T * H * W, C] rows dycoke_ttm takes (no copy)."""
    T, C, H, W = vid.shape
    x = vid.permute(0, 2, 3, 1).reshape(T * H * W, C)
    assert x.is_contiguous()
    return x


@functools.lru_cache(maxsize=None)
def stage1_input(family, T, C, H, W, seed, dtype_name="float32"):
    """Treat the result as read-only: it is shared between tests."""
    dt = DTYPES[dtype_name]
    vid = iid_video(T, C, H, W, seed=seed, dtype=dt) if family == "iid" else synth_video(T, C, H, W, seed=seed, dtype=dt)
    return frames_to_rows(vid)


def ulp_of(v, dt):
    """Spacing of the 16-bit format `dt` at the value v."""
    mant, emin = (7, -126) if dt == torch.bfloat16 else (10, -14)
    e = max(math.frexp(abs(v))[1] - 1, emin) if v != 0.0 else emin
    return 2.0 ** (e - mant)


class LowpReference:
    """16-bit stage 1 as this project documents it: F.cosine_similarity on the CPU in the input dtype, then per pruned frame the
    first k entries of a STABLE ascending sort (ties to the smaller token id; torch.topk leaves them unspecified).
    `near`: tokens within 2 ulps (of the input dtype, at the cut) of their frame's cut value without being equal to it."""

    def __init__(self, x, T, prune):
        self.T, self.P = T, x.shape[0] // T
        self.k = int((1 - prune) * self.P)
        fr = x.reshape(T, self.P, -1)
        self.sims, self.keep, self.cut, self.tol = {}, {}, {}, {}
        self.near = self.kept = 0
        for f in range(T):
            partner = D.pruning_partner(f, T)
            if partner is None:
                continue
            s = F.cosine_similarity(fr[partner], fr[f], dim=1)
            self.sims[f] = s
            self.keep[f] = torch.sort(s.float(), stable=True)[1][:self.k]
            self.kept += self.k
            if self.k:
                cut = float(s[self.keep[f][-1]])
                self.cut[f], self.tol[f] = cut, 2 * ulp_of(cut, x.dtype)
                d = (s.double() - cut).abs()
                self.near += int(((d <= self.tol[f]) & (d > 0)).sum())

    def check(self, out, idx, x):
        """Rows bit-exact; whole frames complete and in order; the kept set of a pruned frame may differ from the reference's only
        in tokens within 2 ulps of the cut, and in at most max(1, near) tokens over the case.  Returns the number that differ."""
        P, k = self.P, self.k
        assert out.dtype == x.dtype and idx.dtype == torch.int64
        assert idx.numel() == sum(k if f in self.keep else P for f in range(self.T)) and out.shape == (idx.numel(), x.shape[1])
        assert int(idx.min()) >= 0 and int(idx.max()) < x.shape[0]
        assert torch.equal(out.view(torch.int16), x[idx].view(torch.int16)), "rows are not bit-exact copies"
        differ, pos = 0, 0
        for f in range(self.T):
            n = k if f in self.keep else P
            got = idx[pos:pos + n]
            pos += n
            assert bool((got // P == f).all()), f"frame {f}: a row of another frame"
            got = (got % P).tolist()
            if f not in self.keep:
                assert got == list(range(P)), f"frame {f} is kept whole"
                continue
            exp = self.keep[f].tolist()
            assert len(set(got)) == k, f"frame {f}: repeated token"
            s = self.sims[f].double()
            for p in set(got) ^ set(exp):
                assert abs(float(s[p]) - self.cut[f]) <= self.tol[f], (f, p, float(s[p]), self.cut[f], self.tol[f])
            differ += len(set(got) - set(exp))
        assert differ <= max(1, self.near), f"{differ} kept tokens differ, {self.near} lie within 2 ulps of a cut"
        return differ


@functools.lru_cache(maxsize=None)
def lowp_reference(C, family, seed, dtype_name):
    x = stage1_input(family, WIDTH_T, C, WIDTH_SIDE, WIDTH_SIDE, seed, dtype_name)
    return x, LowpReference(x, WIDTH_T, WIDTH_PRUNE)


# ---------------------------------------------------------------------------------------------------------------------------------
# stage 1: degenerate clips, pinned by tests/golden/dycod_*.npz (the reference's dycoke_ttm, make_golden_dycoke.py)
# ---------------------------------------------------------------------------------------------------------------------------------
DEG_T, DEG_SIDE, DEG_C = 6, 14, 16                    # P = 196; frames 1, 3, 5 pruned in pass 1, frame 2 in pass 2 (against 0)
NAN, INF = float("nan"), float("inf")


def _inf_elem(m):
    m[3, 50, 3] = INF                                  # norm inf, inf / inf: one NaN similarity in frame 3


def _nan_elem(m):
    m[3, 50, 3] = NAN


def _nan_five(m):
    for p, c in ((7, 0), (50, 3), (51, 15), (120, 8), (195, 1)):
        m[3, p, c] = NAN


def _nan_partner(m):
    m[0, 50, 3] = NAN                                  # frame 0 is the partner of frame 1 (pass 1) and of frame 2 (pass 2)


def _zero_token(m):
    m[3, 50] = 0                                       # similarity exactly 0
    m[2, 60] = 0                                       # seen by the pass-2 pair as the pruned side, by pair (2, 3) as the partner


def _dup_frames(m):
    m[3] = m[2]                                        # every similarity of frame 3 is 1 up to rounding


def _few_finite(m):
    m[3, torch.arange(196) % 4 != 0, 5] = NAN          # 49 finite similarities in frame 3, k = 98


# name -> (edit of the [T, P, C] memory, prune ratio)
DEGENERATE = {
    "inf_elem": (_inf_elem, 0.7),
    "nan_elem": (_nan_elem, 0.7),
    "nan_five": (_nan_five, 0.7),
    "nan_partner": (_nan_partner, 0.7),
    "zero_token": (_zero_token, 0.7),
    "dup_frames": (_dup_frames, 0.7),
    "few_finite": (_few_finite, 0.5),
}
DEG_DTYPES = ("float32", "bfloat16")
# the clips whose expected output changes with the NaN rule of k_dycoke_select (the others hold no non-finite similarity)
DEG_NONFINITE = ("inf_elem", "nan_elem", "nan_five", "nan_partner", "few_finite")


def degenerate_ids():
    return [f"dycod_{name}_{SHORT[d]}" for name in DEGENERATE for d in DEG_DTYPES]


def build_degenerate(name, dtype_name):
    """synth-v1 plus 1e-3 noise (no repeated tokens, as the dyc_* vectors), edited in float32, then rounded to the dtype."""
    P = DEG_SIDE ** 2
    x = frames_to_rows(synth_video(DEG_T, DEG_C, DEG_SIDE, DEG_SIDE, seed=21)).clone()
    x += 1e-3 * torch.randn(x.shape, generator=torch.Generator().manual_seed(121))
    DEGENERATE[name][0](x.view(DEG_T, P, DEG_C))
    return x.to(DTYPES[dtype_name])


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def save_dycod(fid, meta, x, feat, idx):
    """The storage layout of dyc_*.npz (meta, x, feat, idx); 16-bit tensors as their int16 bit patterns, as dyc16_*.npz."""
    raw = (lambda t: t.numpy()) if x.dtype == torch.float32 else (lambda t: _bits(t).numpy())
    np.savez_compressed(os.path.join(GOLDEN_DIR, fid + ".npz"), meta=json.dumps(meta), x=raw(x), feat=raw(feat), idx=idx.numpy())


def load_dycod(fid):
    z = np.load(os.path.join(GOLDEN_DIR, fid + ".npz"))
    meta = json.loads(str(z["meta"]))
    dt = DTYPES[meta["dtype"]]
    cvt = (lambda a: torch.from_numpy(a)) if dt == torch.float32 else (lambda a: torch.from_numpy(a).view(dt))
    return meta, cvt(z["x"]), cvt(z["feat"]), torch.from_numpy(z["idx"])


def bits_equal(a, b):
    """Bit-equal outside NaN, NaN at the same places (a copied NaN keeps its payload, one made by arithmetic need not)."""
    na, nb = torch.isnan(a.float()), torch.isnan(b.float())
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(na, nb) and torch.equal(_bits(a)[~na], _bits(b)[~nb])


def check_degenerate(out, idx, x, exp_idx, sims, T, P, k):
    """What topk(largest=False) does with non-finite similarities, as requirements on (out, idx) for the input x:
      * no pad id: every id of frame f lies in [f P, (f + 1) P), whole frames are complete and in order;
      * a pruned frame keeps min(k, finite) tokens with a finite similarity: none with a non-finite one while a finite one is left out;
      * those, in their order, equal the fixture's, except between tokens whose similarities differ by < 1e-6 (summation order);
      * the rest are distinct tokens of that frame with a non-finite similarity;
      * rows are copies of the chosen tokens."""
    assert idx.dtype == torch.int64 and idx.shape == exp_idx.shape and out.shape == (idx.numel(), x.shape[1]) and out.dtype == x.dtype
    pos = 0
    for f in range(T):
        n = k if f in sims else P
        got, exp = idx[pos:pos + n], exp_idx[pos:pos + n]
        pos += n
        assert bool(((got >= f * P) & (got < (f + 1) * P)).all()), f"frame {f}: ids outside the frame: {got[(got // P) != f][:4].tolist()}"
        got, exp = (got % P).tolist(), (exp % P).tolist()
        if f not in sims:
            assert got == list(range(P)), f"frame {f} is kept whole"
            continue
        s = sims[f].double()
        fin = torch.isfinite(s)
        want_fin = min(k, int(fin.sum()))
        got_fin, exp_fin = [p for p in got if fin[p]], [p for p in exp if fin[p]]
        assert len(exp_fin) == want_fin, "the fixture itself keeps a non-finite token too early"
        assert len(got_fin) == want_fin, f"frame {f}: {k - len(got_fin)} tokens with a non-finite similarity kept, {k - want_fin} expected"
        for a, b in zip(got_fin, exp_fin):
            assert a == b or abs(float(s[a]) - float(s[b])) < 1e-6, (f, a, b, float(s[a]), float(s[b]))
        rest = [p for p in got if not fin[p]]
        assert len(set(got)) == k and len(rest) == k - want_fin, f"frame {f}: repeated token"
    assert bits_equal(out, x[idx]), "rows are not copies of the chosen tokens"


def replay_select(sim, k, nan_as_inf):
    """k_dycoke_select's bitonic network on the CPU (same padding, same comparison, same exchange order), with or without the NaN
    rule of its load.  sim: float32 numpy [P] -> the first k token ids."""
    P, npad = len(sim), 1
    while npad < P:
        npad <<= 1
    key = np.full(npad, np.inf, np.float32)
    key[:P] = sim
    if nan_as_inf:
        key[np.isnan(key)] = np.inf
    val = np.full(npad, 0x7fffffff, np.int64)
    val[:P] = np.arange(P)
    i = np.arange(npad)
    size = 2
    while size <= npad:
        stride = size >> 1
        while stride > 0:
            lo = i[(i ^ stride) > i]
            hi = lo ^ stride
            with np.errstate(invalid="ignore"):
                gt = (key[lo] > key[hi]) | ((key[lo] == key[hi]) & (val[lo] > val[hi]))
            swap = gt == ((lo & size) == 0)
            a, b = lo[swap], hi[swap]
            key[a], key[b] = key[b].copy(), key[a].copy()
            val[a], val[b] = val[b].copy(), val[a].copy()
            stride >>= 1
        size <<= 1
    return torch.from_numpy(val[:k].copy())


# ---------------------------------------------------------------------------------------------------------------------------------
# stage 2: group sizes (the `g0 += kDecGmax` sweep of k_dec_logits / k_dec_gathered, kDecGmax = 8)
# ---------------------------------------------------------------------------------------------------------------------------------
GROUP_HEADS = [
    (1, 1),      # G = 1: one sweep, gn = 1, a single head in all
    (8, 8),      # G = 1 on eight KV heads (blockIdx.y)
    (9, 1),      # G = 9: second sweep with gn = 1
    (12, 1),     # G = 12 (MQA): second sweep with gn = 4
    (32, 2),     # G = 16: two full sweeps
    (40, 8),     # G = 5: one partial sweep
    (256, 1),    # G = 256: 32 sweeps, the kDecMaxHq limit of k_dec_score's sM / sS
]
GROUP_TOO_MANY = (257, 1)
GROUP_LKS = (33, 257, 1000)


def group_cases():
    """(dtype, Hq, Hkv, D, Lk): every head shape with D in {64, 128} and the three dtypes, Lk cycled (not crossed)."""
    cases, n = [], 0
    for dt in DTYPES.values():
        for Dh in (64, 128):
            for Hq, Hkv in GROUP_HEADS:
                cases.append((dt, Hq, Hkv, Dh, GROUP_LKS[n % 3]))
                n += 1
    return cases


# ---------------------------------------------------------------------------------------------------------------------------------
# stage 2: the peaked family
# ---------------------------------------------------------------------------------------------------------------------------------
FLOOR = 2.0 ** -100        # scores below it are not held to a relative bound (float32 underflows at 2^-149 / the largest term)


def peaked_qkv(dt, Hq, Hkv, Dh, Lk, seed, sigma, sink, device="cpu"):
    """Gaussian q; Gaussian K times `sigma` (the scaled logits q.k / sqrt(D) then spread over about +-3 sigma); K row 0 of every KV
    head replaced by `sink` times the unit mean query direction of its group; Gaussian V.  All rounded to `dt`.
    A head aligned with that direction has the sink logit sink |q| / sqrt(D), about `sink`: that is every head where a group is one
    head.  In a group of G heads the alignment is about 1 / sqrt(G) with a scatter of 1 / sqrt(D) from head to head, so the heads
    disagree on how much of their mass the sink takes: from nearly all of it to nearly none."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(1, Hq, 1, Dh, generator=g, dtype=torch.float64)
    k = torch.randn(1, Hkv, Lk, Dh, generator=g, dtype=torch.float64) * sigma
    v = torch.randn(1, Hkv, Lk, Dh, generator=g, dtype=torch.float64)
    mean_q = q.reshape(Hkv, Hq // Hkv, Dh).mean(1)                       # [Hkv, D]
    k[0, :, 0] = sink * mean_q / mean_q.norm(dim=-1, keepdim=True)
    return tuple(t.to(dt).to(device) for t in (q, k, v))


PEAKED_SHAPES = [(32, 2, 128, 257), (12, 1, 64, 1000), (28, 4, 128, 4097), (9, 1, 64, 129)]
PEAKED_LEVELS = [(4.0, 30.0), (8.0, 60.0), (12.0, 200.0)]


# Seeds of three band cases: drawn again until the reference's relative gap at the cut of both windows was above 3e-3; the first
# draws had 5e-4 to 9e-4, too close to ten times the allowance for the band test to be about the kernel.
PEAKED_SEEDS = {(0, 0): 740, (2, 0): 906, (2, 1): 867}


def peaked_cases():
    """(dtype, Hq, Hkv, D, Lk, seed, sigma, sink): shapes x levels, the dtype cycled."""
    cases, dts = [], list(DTYPES.values())
    for i, (Hq, Hkv, Dh, Lk) in enumerate(PEAKED_SHAPES):
        for j, (sigma, sink) in enumerate(PEAKED_LEVELS):
            cases.append((dts[(i + j) % 3], Hq, Hkv, Dh, Lk, PEAKED_SEEDS.get((i, j), 700 + 3 * i + j), sigma, sink))
    return cases


PEAKED_CASES = peaked_cases()
# every head has the same sink logit (G = 1), 200 above a spread of ~4: the other scores underflow float32
SATURATED_CASE = (torch.float32, 2, 2, 64, 257, 750, 4.0, 200.0)
# the band test: the (4, 30) and (8, 60) levels of every shape, windows [1, Lk) and [0, Lk), num_keep = window // 5
BAND_CASES = [c for c in PEAKED_CASES if c[7] < 100.0]
BAND_STARTS = (1, 0)


def scores64(q, k, Dh):
    return R.decode_attn_scores_ref(q.double(), k.double(), Dh ** -0.5)


def peaked_score_allowance(device="cpu"):
    """(largest relative deviation of the float32 restatement on `device` from the float64 one over PEAKED_CASES and the saturated
    case, over entries whose float64 score is at least FLOOR; 4 x that: the project's margin for another summation order)."""
    worst = 0.0
    for dt, Hq, Hkv, Dh, Lk, seed, sigma, sink in PEAKED_CASES + [SATURATED_CASE]:
        q, k, _ = peaked_qkv(dt, Hq, Hkv, Dh, Lk, seed, sigma, sink, device)
        ref = scores64(q, k, Dh)
        own = R.decode_attn_scores_ref(q.float(), k.float(), Dh ** -0.5).double()
        live = ref >= FLOOR
        worst = max(worst, float(((own - ref).abs() / ref)[live].max()))
    return worst, 4 * worst


def band_geometry(Lk, start):
    """(n0, num_keep) of the band test: the window [start, Lk), a fifth of it kept."""
    n0 = Lk - start
    return n0, R.num_keep_of(n0, 0.8)


def cut_gap(s64, start, n0, num_keep):
    """(theta, relative gap between the num_keep-th and the next largest float64 score of the window)."""
    top = torch.sort(s64[start:start + n0], descending=True)[0]
    theta = float(top[num_keep - 1])
    return theta, (theta - float(top[num_keep])) / theta


def peaked_keep_lists(Lk):
    return {"dense": torch.arange(Lk), "no_sink": torch.arange(1, Lk), "sink_and_far_tile": torch.tensor([0] + list(range(Lk - 5, Lk))),
            "single": torch.tensor([Lk // 2])}


def check_keep_well_formed(keep, Lk, start, n0, num_keep):
    """Right length, prefix and tail intact, window ids ascending, distinct and inside the window."""
    tail = max(Lk - start - n0, 0)
    keep = keep.tolist()
    assert len(keep) == start + num_keep + tail
    assert keep[:start] == list(range(start)) and keep[start + num_keep:] == list(range(start + n0, Lk))
    win = keep[start:start + num_keep]
    assert all(a < b for a, b in zip(win, win[1:])), "window ids are not strictly ascending"
    assert not win or (win[0] >= start and win[-1] < min(start + n0, Lk))


# ---------------------------------------------------------------------------------------------------------------------------------
# stage 2: a non-finite cache row that is alone in its tile
# ---------------------------------------------------------------------------------------------------------------------------------
def tile_rows(dt, Dh):
    """DecTile<T, D>::ROWS: kDecRpg * kDecThreads / (lanes per row) = 32 (float32, 128), 64, 128 (16-bit, 64)."""
    return 4 * 256 // (Dh * torch.finfo(dt).bits // 8 // 16)


LONE_LK = 257              # 257 % ROWS == 1 for every ROWS: row 256, the row decode has just written, is alone in the last tile
LONE_ROW = LONE_LK - 1
# what the row holds: (element, value) pairs.  A NaN logit for every head; +Inf alone gives +-inf logits by the sign of q's element
LONE_EDITS = {"nan_and_inf": ((3, NAN), (9, INF)), "nan": ((3, NAN),), "inf": ((9, INF),)}


def lone_cases():
    """(dtype, Hq, Hkv, D): every dtype and D (every ROWS), group sizes of one and of two sweeps."""
    heads = ((4, 2), (12, 1))
    return [(dt, *heads[(i + j) % 2], Dh) for i, dt in enumerate(DTYPES.values()) for j, Dh in enumerate((64, 128))]


def lone_keep_lists(dt, Dh):
    """Keep lists whose last tile holds nothing valid but LONE_ROW: one full tile of finite rows, then that row alone; the same with
    skipped entries around it; and that row in the first tile, alone, before a full tile of finite rows."""
    rows = tile_rows(dt, Dh)
    full = list(range(5, 5 + rows))
    return {"full_tile_then_lone": torch.tensor(full + [LONE_ROW], dtype=torch.int32),
            "lone_among_skipped": torch.tensor(full + [-1, LONE_ROW, LONE_LK], dtype=torch.int32),
            "lone_tile_first": torch.tensor([LONE_ROW] + [-1] * (rows - 1) + full, dtype=torch.int32)}


# ---------------------------------------------------------------------------------------------------------------------------------
# stage 2: keep lists with skipped entries (Lk = 300, float32, D = 128: tiles of 32 keep entries)
# ---------------------------------------------------------------------------------------------------------------------------------
SKIP_LK = 300


def skip_keep_lists():
    """name -> (keep list with entries outside [0, Lk), the valid ids alone).  A: five skipped entries scattered among 40 valid ids.
    B: 32 skipped entries first, a whole tile of k_dec_gathered<float, 128>, then the 40 valid ids."""
    valid = list(range(3, 300, 7))[:40]
    a = list(valid)
    for at, bad in ((0, -1), (9, SKIP_LK), (20, -1), (33, SKIP_LK), (44, -1)):
        a.insert(at, bad)
    b = [-1] * 32 + valid
    assert len(a) == 45 and len(valid) == 40
    return {"A_scattered": (torch.tensor(a, dtype=torch.int32), torch.tensor(valid, dtype=torch.int32)),
            "B_whole_tile": (torch.tensor(b, dtype=torch.int32), torch.tensor(valid, dtype=torch.int32))}
