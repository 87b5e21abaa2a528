"""Off-distribution inputs for the quadtree (STTM) path: near-threshold ladders, degenerate clips, decision decoders and a
NaN-aware comparison.  Shared by tests/test_offdist_cpu.py, tests/test_hip_offdist.py, tests/golden/make_golden_offdist.py and
tools/near_threshold_ladder.py.  Everything here runs on the CPU; nothing imports the device library.

Ladders.  A ladder video places the decisions of one level a known distance from the threshold: `delta` in +-{1e-7 .. 1e-4}
(the rungs).  For each decision the float64 similarity of the rows the reference compares and the oracle's own fp32 similarity are
computed here; `eps = 2 * max |sim_fp32 - sim_float64|` over the video is the band inside which a different summation order may
legitimately flip a decision (a device sum and the reference sum may err in opposite directions, hence the 2).  Outside the band
the device, the oracle and float64 must agree.
"""
import functools
import hashlib
import json
import os

import numpy as np
import torch

from oracle import sttm_oracle as O
from sttm_amd.synth import synth_video
from tests._golden import GOLDEN_DIR, _t

RUNGS = (1e-7, 1e-6, 1e-5, 1e-4)
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
FP32_TOL = 1e-5          # the project's bars (BASELINE.json north star), made relative to max(1, |expected|)
LOWP_TOL = 2 ** -7


# ----------------------------------------------------------------------------------------------
# NaN-aware comparison
# ----------------------------------------------------------------------------------------------

def check_nan_aware(out, exp, what=""):
    """tlbr and num_patches exact; NaN, +Inf and -Inf at identical positions; finite features within
    1e-5 * max(1, |exp|) (fp32) or 2^-7 * max(1, |exp|) (16-bit)."""
    feat, npatch, tlbr = (v.cpu() for v in out[:3])
    efeat, enpatch, etlbr = exp[:3]
    assert tlbr.dtype == torch.int32 and npatch.dtype == torch.int32 and feat.dtype == efeat.dtype, f"{what}: dtypes"
    assert tlbr.shape == etlbr.shape, f"{what}: N'={tlbr.shape[0]} expected {etlbr.shape[0]}"
    if not torch.equal(tlbr, etlbr):
        bad = (tlbr != etlbr).any(dim=1).nonzero().flatten()
        raise AssertionError(f"{what}: tlbr differs at rows {bad[:5].tolist()}: {tlbr[bad[0]].tolist()} vs {etlbr[bad[0]].tolist()}")
    assert torch.equal(npatch, enpatch), f"{what}: num_patches differ"
    g, e = feat.float(), efeat.float()
    for name, fn in (("NaN", torch.isnan), ("+Inf", torch.isposinf), ("-Inf", torch.isneginf)):
        a, b = fn(g), fn(e)
        if not torch.equal(a, b):
            bad = (a != b).nonzero()
            raise AssertionError(f"{what}: {name} positions differ ({int(a.sum())} vs {int(b.sum())} expected), first at {bad[0].tolist()}: "
                                 f"got {float(g[tuple(bad[0])])}, expected {float(e[tuple(bad[0])])}")
    fin = torch.isfinite(e)
    tol = FP32_TOL if feat.dtype == torch.float32 else LOWP_TOL
    err = ((g - e).abs() / e.abs().clamp_min(1.0))[fin]
    worst = float(err.max()) if err.numel() else 0.0
    assert worst <= tol, f"{what}: finite feature max relative err {worst:.3e} > {tol:.1e}"


def bits_equal_nan_aware(got, exp):
    """CPU oracle against a fixture: NaN positions identical, everything else (finite values, +-Inf) bit-equal."""
    if got.dtype != exp.dtype or got.shape != exp.shape:
        return False
    gn, en = torch.isnan(got.float()), torch.isnan(exp.float())
    if not torch.equal(gn, en):
        return False
    view = torch.int32 if got.dtype == torch.float32 else torch.int16
    return torch.equal(got.contiguous().view(view)[~gn], exp.contiguous().view(view)[~en])


# ----------------------------------------------------------------------------------------------
# degenerate clips
# ----------------------------------------------------------------------------------------------

def _base(dtype):
    return synth_video(6, 32, 14, 14, seed=0, dtype=dtype)


def _edit(fn):
    def build(dtype):
        x = _base(dtype)
        m = x.permute(0, 2, 3, 1)                 # the [T, H, W, C] memory
        assert m.is_contiguous()
        fn(m)
        return x
    return build


def _zero_tokens(m):
    m[0, 13, 13] = 0
    m[4, 0, 0] = 0
    m[2, 5, 7] = 0


def _zero_frame(m):
    m[3] = 0


def _zero_block(m):
    m[:, 6:8, 6:8] = 0


def _zero_video(m):
    m.zero_()


def _dup_frames(m):
    m[3] = m[2]
    m[4] = m[2]


def _static(m):
    m[:] = m[0].clone()


def _const(m):
    m[:] = m[0, 0, 0].clone()


def _nan_elem(m):
    m[2, 5, 7, 3] = float("nan")


def _inf_elem(m):
    m[2, 5, 7, 3] = float("inf")


def _inf_block(m):
    # one 2x2 leaf block (a level-1 cell of the 14x14 -> 7x7 pyramid) of identical tokens, +Inf in one channel: without the Inf the
    # block would stop (cosine 1); the reference's NaN similarity splits it to four leaves
    m[1, 4:6, 8:10] = m[1, 4, 8].clone()
    m[1, 4:6, 8:10, 5] = float("inf")


def _pm_inf(m):
    m[2, 5, 7, 3] = float("-inf")
    m[2, 5, 7, 4] = float("inf")


def _scaled(k):
    def fn(m):
        m.mul_(2.0 ** k)                            # exact in every dtype used here (no over- or underflow of an element)
    return fn


ALLMERGE_CHANNELS = (5, 20, 37, 60)


def allmerge_video(T, dtype, seed=7):
    """synth-v1 with four channels overwritten by 100 * (1 + 0.02 * randn): every cosine is ~1, everything merges into the 16 roots."""
    x = synth_video(T, 64, 14, 14, seed=seed, dtype=torch.float32)
    m = x.permute(0, 2, 3, 1)
    g = torch.Generator().manual_seed(seed + 1000)
    for ch in ALLMERGE_CHANNELS:
        m[..., ch] = 100.0 * (1.0 + 0.02 * torch.randn(T, 14, 14, generator=g))
    return m.to(dtype).permute(0, 3, 1, 2)


def _allmerge(T):
    return lambda dtype: allmerge_video(T, dtype)


STD = dict(threshold=0.85, temporal_thresh=0.55, root_level=1)

# name -> (builder(dtype) -> [T, C, H, W] view of [T, H, W, C] memory, keyword arguments, dtypes with a fixture, input stored?)
# Inputs too large for a committed file (T >= 32 clips) are rebuilt by the builder and verified against a digest in the fixture.
DEGENERATE = {
    "zero_tokens": (_edit(_zero_tokens), STD, ("float32", "bfloat16"), True),
    "zero_frame": (_edit(_zero_frame), STD, ("float32", "bfloat16"), True),
    "zero_block": (_edit(_zero_block), STD, ("float32", "bfloat16"), True),
    "zero_video": (_edit(_zero_video), STD, ("float32", "bfloat16"), True),
    "dup_frames": (_edit(_dup_frames), STD, ("float32", "bfloat16"), True),
    "static": (_edit(_static), STD, ("float32", "bfloat16"), True),
    "const": (_edit(_const), STD, ("float32", "bfloat16"), True),
    "const_thr1": (_edit(_const), dict(threshold=1.0, temporal_thresh=1.0, root_level=1), ("float32", "bfloat16"), True),
    "nan_elem": (_edit(_nan_elem), STD, ("float32", "bfloat16"), True),
    "inf_elem": (_edit(_inf_elem), STD, ("float32", "bfloat16"), True),
    "inf_block": (_edit(_inf_block), STD, ("float32", "bfloat16"), True),
    "pm_inf": (_edit(_pm_inf), STD, ("float32", "bfloat16"), True),
    "scale_p40": (_edit(_scaled(40)), STD, ("float32", "bfloat16"), True),
    "scale_m40": (_edit(_scaled(-40)), STD, ("float32", "bfloat16"), True),
    "scale_m70": (_edit(_scaled(-70)), STD, ("float32", "bfloat16"), True),
    "scale_p62": (_edit(_scaled(62)), STD, ("float32", "bfloat16"), True),
    "allmerge": (_allmerge(32), STD, ("float32", "bfloat16", "float16"), False),
    "allmerge_w": (_allmerge(32), dict(STD, weighted_avg=True), ("float32", "bfloat16", "float16"), False),
    # sum pooling: a root cell's node is ~100 * 16 in the four large channels and 48 of them are added in float16 -> past 65 504
    "overflow_t48_w": (_allmerge(48), dict(STD, weighted_avg=True), ("float16",), False),
    "static_slow": (_edit(_static), dict(STD, slow_ver=True), ("float32", "bfloat16"), True),
    "dup_frames_slow": (_edit(_dup_frames), dict(STD, slow_ver=True), ("float32", "bfloat16"), True),
}
SHORT = {"float32": "f32", "bfloat16": "bf16", "float16": "f16"}


def degenerate_ids():
    return [f"od_{name}_{SHORT[d]}" for name, (_, _, dts, _) in DEGENERATE.items() for d in dts]


def build_degenerate(name, dtype):
    return DEGENERATE[name][0](dtype)


def digest(x):
    mem = x.permute(0, 2, 3, 1).contiguous()
    raw = mem.view(torch.int16 if mem.element_size() == 2 else torch.int32).numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()


def load_od(fid):
    """One od_*.npz fixture -> dict(name, meta, x, feat, npatch, tlbr).  The input is read from the file, or, where the file carries
    only its digest, rebuilt by the builder and checked against it."""
    z = np.load(os.path.join(GOLDEN_DIR, fid + ".npz"))
    meta = json.loads(str(z["meta"]))
    dname = meta["dtype"]
    if "x_thwc" in z:
        x = _t(z["x_thwc"], dname).permute(0, 3, 1, 2)
    else:
        x = build_degenerate(meta["case"], DTYPES[dname])
        assert digest(x) == meta["x_sha256"], f"{fid}: the rebuilt input differs from the one the fixture was made from"
    return dict(name=meta["name"], meta=meta, x=x, feat=_t(z["feat"], dname), npatch=torch.from_numpy(z["npatch"]),
                tlbr=torch.from_numpy(z["tlbr"]))


OCTREE_KINDS = ("inf_cube", "scale_p62", "zero_cube", "nan_elem")
OCTREE_THR, OCTREE_ROOT = 0.8, 0


def build_octree_degenerate(kind):
    """The octree baseline's degenerate clips (T=16, 8x8, C=32, fp32): a 2x2x2 cube of identical tokens with +Inf in one channel
    (the reference's NaN similarity splits it), norms past fp32 overflow (similarity 0: nothing stops), an all-zero cube, one NaN."""
    x = synth_video(16, 32, 8, 8, seed=11, c=0.15, p_static=0.7)
    m = x.permute(0, 2, 3, 1)
    if kind == "inf_cube":
        m[2:4, 4:6, 2:4] = m[2, 4, 2].clone()
        m[2:4, 4:6, 2:4, 5] = float("inf")
    elif kind == "scale_p62":
        m.mul_(2.0 ** 62)
    elif kind == "zero_cube":
        m[8:10, 0:2, 6:8] = 0
    elif kind == "nan_elem":
        m[9, 3, 3, 7] = float("nan")
    else:
        raise ValueError(kind)
    return x


def load_odoct(kind):
    """tests/golden/odoct_<kind>.npz (the reference's get_octree_features on build_octree_degenerate(kind)) -> (x, features)."""
    z = np.load(os.path.join(GOLDEN_DIR, f"odoct_{kind}.npz"))
    return _t(z["x_thwc"], "float32").permute(0, 3, 1, 2), _t(z["feat"], "float32")


def check_features_nan_aware(out, exp, what, tol=FP32_TOL):
    out, exp = out.cpu(), exp.cpu()
    assert out.shape == exp.shape, f"{what}: {out.shape[0]} tokens, expected {exp.shape[0]}"
    for fn in (torch.isnan, torch.isposinf, torch.isneginf):
        assert torch.equal(fn(out), fn(exp)), f"{what}: {fn.__name__} positions differ"
    fin = torch.isfinite(exp)
    err = ((out - exp).abs() / exp.abs().clamp_min(1.0))[fin]
    assert (float(err.max()) if err.numel() else 0.0) <= tol, f"{what}: finite features differ"


def od_kwargs(meta):
    kw = dict(meta["kw"])
    return kw.pop("threshold"), kw


# ----------------------------------------------------------------------------------------------
# ladders
# ----------------------------------------------------------------------------------------------

def _rand64(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _perp_same_norm(a, g):
    """b with b . a = 0 and |b| = |a| along the last axis, float64."""
    r = _rand64(g, *a.shape)
    r = r - (r * a).sum(-1, keepdim=True) / (a * a).sum(-1, keepdim=True) * a
    return r * (a.norm(dim=-1, keepdim=True) / r.norm(dim=-1, keepdim=True))


def _rung_table(g, *shape):
    idx = torch.randint(0, 2 * len(RUNGS), shape, generator=g)
    mag = torch.tensor(RUNGS, dtype=torch.float64)[idx % len(RUNGS)]
    return torch.where(idx < len(RUNGS), mag, -mag)


def spatial_ladder_video(T, C, thr, seed, dtype=torch.float32, H=16, W=16, head_dim=None):
    """Every 2x2 leaf block is (u + s v, u - s/3 v, u - s/3 v, u - s/3 v) with v perpendicular to u, |v| = |u| and
    s = sqrt(1 / (thr + delta)^2 - 1): the block's mean is u, one leaf has cosine thr + delta with it, the other three are far
    above the threshold.  The slot of the odd leaf is drawn per block.  u is independent per block, so every level above splits.
    With `head_dim` the construction is applied to every head's slice, so the per-head mean sits at thr + delta too.
    Returns (x [T, C, H, W] view of channels-last memory, delta [T, H/2, W/2])."""
    assert H % 2 == 0 and W % 2 == 0
    g = torch.Generator().manual_seed(int(seed))
    hd = C if head_dim is None else head_dim
    nh = C // hd
    u = _rand64(g, T, H // 2, W // 2, nh, hd)
    v = _perp_same_norm(u, g)
    delta = _rung_table(g, T, H // 2, W // 2)
    s = torch.sqrt(1.0 / (thr + delta) ** 2 - 1.0)[..., None, None]
    odd = torch.randint(0, 4, (T, H // 2, W // 2), generator=g)
    x = torch.empty(T, H, W, nh, hd, dtype=torch.float64)
    for k in range(4):
        leaf = torch.where((odd == k)[..., None, None], u + s * v, u - s / 3 * v)
        x[:, (k >> 1)::2, (k & 1)::2] = leaf
    x = x.reshape(T, H, W, C).to(dtype)
    return x.permute(0, 3, 1, 2), delta


def temporal_ladder_video(T, C, tthr, seed, dtype=torch.float32, H=16, W=16, head_dim=None):
    """Even frames are iid normal; odd frame t is scale * (c a + sqrt(1 - c^2) b) per token with a = the token of the same cell in
    frame t-1, b perpendicular to a with |b| = |a|, c = tthr + delta and scale in [0.5, 1.5].  Frame t+1 is unrelated again, so a
    flipped pair changes that pair only.  Returns (x, delta [T//2, H, W]) for the pairs (2i, y, x) -> (2i+1, y, x)."""
    g = torch.Generator().manual_seed(int(seed))
    hd = C if head_dim is None else head_dim
    nh = C // hd
    x = _rand64(g, T, H, W, nh, hd)
    delta = _rung_table(g, T // 2, H, W)
    c = (tthr + delta)[..., None, None]
    for i in range(T // 2):
        a = x[2 * i]
        b = _perp_same_norm(a, g)
        scale = 0.5 + torch.rand(H, W, 1, 1, generator=g, dtype=torch.float64)
        x[2 * i + 1] = scale * (c[i] * a + torch.sqrt(1 - c[i] ** 2) * b)
    x = x.reshape(T, H, W, C).to(dtype)
    return x.permute(0, 3, 1, 2), delta


def _cos64(p, c, head_dim):
    """F.cosine_similarity's formula in float64 on [n, k, C] rows (eps clamp included; it never binds here)."""
    if head_dim is not None:
        p = p.reshape(*p.shape[:-1], -1, head_dim)
        c = c.reshape(*c.shape[:-1], -1, head_dim)
    s = (p * c).sum(-1) / (p.norm(dim=-1).clamp_min(O.EPS_SPATIAL) * c.norm(dim=-1).clamp_min(O.EPS_SPATIAL))
    return s.mean(-1) if head_dim is not None else s


def spatial_ladder_sims(x, head_dim=None):
    """The leaf-level decisions of a spatial ladder video: for every 2x2 block the four similarities of the level above the leaves
    (as the oracle's pyramid forms it, in the input dtype) with its four children, in float64 and as the oracle computes them in
    fp32.  Returns (sim64, sim32) [T, H/2, W/2, 4]."""
    m = x.permute(0, 2, 3, 1)
    T, H, W, C = m.shape
    parent = O.pool_level(m, "avg")                                   # [T, H/2, W/2, C] input dtype
    kids = torch.stack([m[:, (k >> 1)::2, (k & 1)::2] for k in range(4)], dim=3)      # [T, H/2, W/2, 4, C]
    p = parent.reshape(-1, 1, C).float()
    c = kids.reshape(-1, 4, C).float()
    sim32 = O._cosine(p, c, head_dim).double()
    sim64 = _cos64(p.double(), c.double(), head_dim)
    return sim64.reshape(T, H // 2, W // 2, 4), sim32.reshape(T, H // 2, W // 2, 4)


def temporal_ladder_sims(x, head_dim=None):
    """The ladder pairs (2i, y, x) -> (2i+1, y, x): float64 and the oracle's fp32 similarity, [T//2, H, W]."""
    m = x.permute(0, 2, 3, 1)
    T, H, W, C = m.shape
    n = T // 2
    rows = m[:2 * n].reshape(n, 2, H * W, C)
    a, b = rows[:, 0].reshape(-1, C), rows[:, 1].reshape(-1, C)
    both = torch.cat([a, b])
    k = a.shape[0]
    pairs = torch.stack([torch.arange(k), torch.arange(k) + k], dim=1)
    sim32 = O.pair_similarity(O.unit_rows(both, head_dim), pairs).double()
    d = both.double()
    if head_dim is not None:
        d = d.reshape(d.shape[0], -1, head_dim)
    dn = d / (d.norm(dim=-1, keepdim=True) + O.EPS_TEMPORAL)
    s = (dn[:k] * dn[k:]).sum(-1)
    sim64 = s.mean(-1) if s.dim() == 2 else s
    return sim64.reshape(n, H, W), sim32.reshape(n, H, W)


def decode_spatial(tlbr, T, H, W):
    """[T, H/2, W/2] bool: the 2x2 block stopped (one 2x2 box in tlbr) rather than split into four leaves.  Asserts that tlbr
    holds nothing but these two forms, i.e. that every level above split."""
    tl = tlbr.cpu().long()
    hh, ww = tl[:, 3] - tl[:, 1], tl[:, 4] - tl[:, 2]
    two = (hh == 2) & (ww == 2)
    assert bool((two | ((hh == 1) & (ww == 1))).all()), "a ladder video produced a node above the ladder level"
    stop = torch.zeros(T, H // 2, W // 2, dtype=torch.bool)
    b = tl[two]
    stop[b[:, 0], b[:, 1] // 2, b[:, 2] // 2] = True
    assert int(stop.sum()) * 4 + int((~two).sum()) == T * H * W
    return stop


def decode_temporal(tlbr, T, H, W):
    """[T//2, H, W] bool: the pair (2i, y, x) -> (2i+1, y, x) was kept, i.e. box (2i+1, y, x) is absent from tlbr."""
    tl = tlbr.cpu().long()
    assert bool(((tl[:, 3] - tl[:, 1] == 1) & (tl[:, 4] - tl[:, 2] == 1)).all()), "a temporal ladder video merged spatially"
    present = torch.zeros(T, H, W, dtype=torch.bool)
    present[tl[:, 0], tl[:, 1], tl[:, 2]] = True
    assert bool(present[0::2].all()), "an even (unrelated) frame lost a token"
    return ~present[1:2 * (T // 2):2]


class Ladder:
    """One ladder video with its truth: `sim64` / `sim32` of the deciding comparison of every ladder decision, the float64 and the
    oracle-fp32 decisions, and the band `eps`."""

    def __init__(self, kind, T, C, thr, tthr, seed, dtype, H=16, W=16, head_dim=None):
        self.kind, self.T, self.C, self.H, self.W, self.head_dim, self.dtype = kind, T, C, H, W, head_dim, dtype
        self.thr, self.tthr = thr, tthr
        if kind == "spatial":
            self.x, self.delta = spatial_ladder_video(T, C, thr, seed, dtype, H, W, head_dim)
            s64, s32 = spatial_ladder_sims(self.x, head_dim)
            k = s64.argmin(dim=-1, keepdim=True)                     # the slot that decides: the other three are far above
            self.sim64, self.sim32 = s64.gather(-1, k)[..., 0], s32.gather(-1, k)[..., 0]
            self.far = float(s64.scatter(-1, k, 9.0).min())          # the smallest similarity of a non-deciding slot
            self.level = thr
            # Rows of 256 and more channels run the whole pipeline: blocks with independent u stay far below the temporal threshold,
            # so no pair is kept and tlbr still shows the spatial decisions alone (decode_spatial counts the boxes; the CPU test
            # compares with the spatial-only run).  The column walk exists only with the temporal stage on.  At C = 64 unrelated
            # tokens are not far enough apart for that, so those ladders run the spatial stage alone.
            self.run_tthr = tthr if C >= 256 else -1.0
        else:
            self.x, self.delta = temporal_ladder_video(T, C, tthr, seed, dtype, H, W, head_dim)
            self.sim64, self.sim32 = temporal_ladder_sims(self.x, head_dim)
            self.level = tthr
            self.run_tthr = tthr
        # `sim_fp32 >= threshold` compares fp32 numbers: the python threshold is rounded to fp32 first
        self.level32 = float(torch.tensor(self.level, dtype=torch.float32))
        self.eps = 2.0 * float((self.sim32 - self.sim64).abs().max())
        self.want64 = self.sim64 >= self.level32
        self.want32 = self.sim32 >= self.level32
        self.outside = (self.sim64 - self.level32).abs() > self.eps

    def kwargs(self, **extra):
        kw = dict(temporal_thresh=self.run_tthr, root_level=1 if (self.H, self.W) == (16, 16) else 0)
        if self.head_dim is not None:
            kw["head_dim"] = self.head_dim
        kw.update(extra)
        return kw

    def decode(self, tlbr):
        return (decode_spatial if self.kind == "spatial" else decode_temporal)(tlbr, self.T, self.H, self.W)

    def oracle_decisions(self, **extra):
        return self.decode(O.get_quadtree_features(self.x, self.thr, **self.kwargs(**extra))[2])

    def assert_outside_band(self, got, what):
        """1a: every decision further than eps from the threshold equals the float64 decision."""
        bad = (got != self.want64) & self.outside
        if bool(bad.any()):
            i = tuple(bad.nonzero()[0].tolist())
            raise AssertionError(f"{what}: {int(bad.sum())} of {int(self.outside.sum())} decisions outside the band (eps {self.eps:.2e}) "
                                 f"differ from float64; first at {i}: sim64 - thr = {float(self.sim64[i] - self.level32):+.3e}, got "
                                 f"{bool(got[i])}")

    def flips_by_rung(self, got, ref):
        """1d: {rung: (decisions inside the band, of which got != ref)}."""
        out = {}
        inside = ~self.outside
        for r in RUNGS:
            sel = inside & (self.delta.abs() == r)
            out[r] = (int(sel.sum()), int(((got != ref) & sel).sum()))
        return out


@functools.lru_cache(maxsize=None)
def ladder(kind, T, C, thr, tthr, seed, dtype_name="float32", H=16, W=16, head_dim=None):
    return Ladder(kind, T, C, thr, tthr, seed, DTYPES[dtype_name], H, W, head_dim)


PRESETS = ((0.85, 0.55), (0.94, 0.82))

# (kind, T, C, thr, tthr, seed, dtype, H, W, head_dim) of the default path (issue table 1c, first row); the temporal ladder keeps
# C >= 256 so that unrelated tokens stay far below the threshold
DEFAULT_LADDERS = []
for _i, (_thr, _tthr) in enumerate(PRESETS):
    for _d, _cs in (("float32", (64, 1000, 3584)), ("bfloat16", (64, 3584)), ("float16", (64, 3584))):
        for _c in _cs:
            DEFAULT_LADDERS.append(("spatial", 8, _c, _thr, _tthr, 100 + _i, _d, 16, 16, None))
            DEFAULT_LADDERS.append(("temporal", 8, max(_c, 256), _thr, _tthr, 200 + _i, _d, 16, 16, None))


def ladder_id(spec):
    kind, T, C, thr, tthr, seed, d, H, W, hd = spec
    return f"{kind}_{SHORT[d]}_C{C}_{thr}_{tthr}" + (f"_hd{hd}" if hd else "") + (f"_{H}x{W}" if H != 16 else "")

# ladders for the paths with their own decision arithmetic or reduction order (issue table 1c); the switches are set by the GPU test
COLWALK_LADDERS = [("spatial", 8, 1024, 0.85, 0.55, 110, "float32", 16, 16, None), ("temporal", 8, 1024, 0.85, 0.55, 210, "float32", 16, 16, None)]
HEAD_LADDERS = [(k, 8, 512, thr, tthr, s, d, 16, 16, 128) for d in ("float32", "bfloat16")
                for (k, s) in (("spatial", 120), ("temporal", 220)) for (thr, tthr) in PRESETS[:1]]
SLOW_LADDERS = [("temporal", 8, 256, 0.85, 0.55, 230, "float32", 16, 16, None)]
NODES_LADDERS = [("temporal", 8, 256, 0.94, 0.82, 240, "float32", 16, 16, None), ("temporal", 8, 256, 0.85, 0.55, 241, "bfloat16", 16, 16, None)]
BATCH_LADDERS = [("temporal", 8, 256, 0.85, 0.55, 250, "float32", 16, 16, None), ("temporal", 6, 256, 0.85, 0.55, 251, "float32", 16, 16, None),
                 ("temporal", 8, 256, 0.85, 0.55, 252, "float32", 16, 16, None), ("temporal", 6, 256, 0.85, 0.55, 253, "float32", 16, 16, None)]
BATCH_SPATIAL_LADDERS = [("spatial", 8, 256, 0.85, 0.55, 260, "float32", 16, 16, None), ("spatial", 10, 256, 0.85, 0.55, 261, "float32", 16, 16, None),
                         ("spatial", 8, 256, 0.85, 0.55, 262, "float32", 16, 16, None), ("spatial", 10, 256, 0.85, 0.55, 263, "float32", 16, 16, None)]
WIDE_LADDERS = [("spatial", 8, 8192, 0.85, 0.55, 130, "float32", 16, 16, None), ("temporal", 8, 8192, 0.85, 0.55, 231, "float32", 16, 16, None)]
DEEP_LADDERS = [("spatial", 2, 64, 0.85, 0.55, 140, "float32", 64, 64, None)]
ALL_LADDERS = (DEFAULT_LADDERS + COLWALK_LADDERS + HEAD_LADDERS + SLOW_LADDERS + NODES_LADDERS + BATCH_LADDERS + BATCH_SPATIAL_LADDERS
               + WIDE_LADDERS + DEEP_LADDERS)


# ----------------------------------------------------------------------------------------------
# whole-video margins (heavy-tailed family): every decision the oracle takes, with its float64 twin
# ----------------------------------------------------------------------------------------------

class Margins:
    """The oracle's run on one video with, for every decision it took, the fp32 similarity it used and the float64 similarity of
    the same rows.  eps_* = 2 * max |sim_fp32 - sim_float64| per stage.  A spatial parent is decided outside the band when all four
    slots are more than eps above the threshold or one slot is more than eps below it; a candidate pair when it is more than eps
    away from the temporal threshold.  `decisive`: every decision of the video is."""

    def __init__(self, x, thr, tthr, root_level, head_dim=None):
        T, C, H, W = x.shape
        geom = O.Geometry(H, W, root_level)
        h0, w0 = geom.dims[0]
        st = dict(lvl=0, t=torch.arange(T).repeat_interleave(h0 * w0), cell=torch.arange(h0 * w0).repeat(T))
        sp, tp = [], []
        cos32, keep32 = O._cosine, O.keep_similar_pairs

        def cosine(p, c, hd):
            s32 = cos32(p, c, hd)
            sp.append((st["t"], geom.boxes(st["lvl"])[st["cell"]], s32.double(), _cos64(p.double(), c.double(), hd)))
            ids, ok = geom.child_table(st["lvl"])                        # follow spatial_split's own bookkeeping to the next level
            go = (~(s32 >= thr).all(dim=-1))[:, None] & ok[st["cell"]]
            st.update(lvl=st["lvl"] + 1, t=st["t"][:, None].expand(-1, 4)[go], cell=ids[st["cell"]][go])
            return s32

        def keep(rows, pairs, tt, hd=None):
            s32 = O.pair_similarity(O.unit_rows(rows, hd), pairs)
            d = rows.double()
            if hd is not None:
                d = d.reshape(d.shape[0], -1, hd)
            dn = d / (d.norm(dim=-1, keepdim=True) + O.EPS_TEMPORAL)
            s = (dn[pairs[:, 0]] * dn[pairs[:, 1]]).sum(-1)
            tp.append((pairs, s32.double(), s.mean(-1) if s.dim() == 2 else s))
            return pairs[s32 >= tt]

        O._cosine, O.keep_similar_pairs = cosine, keep
        try:
            *self.out, dbg = O.get_quadtree_features(x, thr, tthr, root_level, head_dim=head_dim, return_debug=True)
        finally:
            O._cosine, O.keep_similar_pairs = cos32, keep32
        thr32 = float(torch.tensor(thr, dtype=torch.float32))
        tthr32 = float(torch.tensor(tthr, dtype=torch.float32))
        boxes = []                                                      # [t, y1, x1, y2, x2] of every decision inside the band
        self.eps_sp = 2.0 * max([float((a - b).abs().max()) for _, _, a, b in sp if a.numel()] or [0.0])
        self.n_decisions = 0
        for t, box, _, s64 in sp:
            clear = ((s64 - thr32) > self.eps_sp).all(-1) | ((thr32 - s64) > self.eps_sp).any(-1)
            self.n_decisions += int(clear.numel())
            boxes.append(torch.cat([t[~clear, None].int(), box[~clear]], dim=1))
        self.eps_tp = 0.0
        node_tlbr = dbg["spatial_tlbr"]
        for pairs, s32, s64 in tp:
            if s32.numel():
                self.eps_tp = 2.0 * float((s32 - s64).abs().max())
            near = (s64 - tthr32).abs() <= self.eps_tp
            self.n_decisions += int(near.numel())
            boxes += [node_tlbr[pairs[near, 0]], node_tlbr[pairs[near, 1]]]
        self.band_boxes = torch.cat(boxes) if boxes else torch.zeros(0, 5, dtype=torch.int32)
        self.decisive = self.band_boxes.shape[0] == 0

    def assert_differences_trace_to_the_band(self, tlbr, npatch, what):
        """For a video with decisions inside the band: every node the device and the oracle disagree on (a box only one of them
        has, or a box with another patch count) overlaps the box of a decision inside the band -- a flipped decision changes the
        nodes under its box and, through the label chains, the groups of that column of cells in other frames."""
        mine = {tuple(r): int(n) for r, n in zip(tlbr.cpu().tolist(), npatch.cpu().tolist())}
        ref = {tuple(r): int(n) for r, n in zip(self.out[2].tolist(), self.out[1].tolist())}
        diff = [k for k in set(mine) | set(ref) if mine.get(k) != ref.get(k)]
        bb = self.band_boxes.long()
        for (t, y1, x1, y2, x2) in diff:
            hit = (bb[:, 1] < y2) & (bb[:, 3] > y1) & (bb[:, 2] < x2) & (bb[:, 4] > x1)
            assert bool(hit.any()), f"{what}: node {(t, y1, x1, y2, x2)} differs from the oracle away from every decision inside the band"
        return len(diff)


HEAVY_SETTINGS = ("massive", "crowded")
HEAVY_COMBOS = [(1024, "float32", 0.85, 0.55), (1024, "float32", 0.94, 0.82), (3584, "bfloat16", 0.85, 0.55), (3584, "bfloat16", 0.94, 0.82)]
HEAVY_SEEDS = (0, 1, 2, 3)          # 4 combinations x 4 seeds = 16 videos per setting


@functools.lru_cache(maxsize=None)
def heavy_case(setting, C, dtype_name, thr, tthr, seed):
    from sttm_amd.synth import HEAVY_CROWDED_SCALE, heavy_video
    scale = 100.0 if setting == "massive" else HEAVY_CROWDED_SCALE[C]
    x = heavy_video(16, C, 14, 14, seed=seed, n_massive=6, scale=scale, dtype=DTYPES[dtype_name])
    return x, Margins(x, thr, tthr, 1)
