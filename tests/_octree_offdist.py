"""Off-distribution inputs for the octree baseline: margins of every stop decision, a float64-decided traversal, near-threshold
ladders with a decoder for the row-only output, degenerate clips and the dispatch / shape case table.  Shared by
tests/test_octree_offdist_cpu.py, tests/test_hip_octree_offdist.py and tests/golden/make_golden_octree_offdist.py.  Everything here
runs on the CPU; nothing imports the device library, and the product path never imports this module.

Margins.  The oracle's own pyramid (OC.pool_cube_level) is built for a video; for every (level, cell, slot) -- the slots without a
child, which alias child cell (0, 0, 0) of the cube, included -- the float32 F.cosine_similarity the oracle uses and the float64
similarity of the same rows are computed.  As in tests/_offdist.py, eps = 2 * max |sim32 - sim64| over the video is the band inside
which another summation order may legitimately flip a decision; a decision is in the band when |sim64 - thr| <= eps.
"""
import functools
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import octree_oracle as OC
from oracle import sttm_oracle as O
from sttm_amd.synth import heavy_video, iid_video, synth_video
from tests import _offdist as D
from tests._golden import GOLDEN_DIR, _t

SLOTS = [(s >> 2, (s >> 1) & 1, s & 1) for s in range(8)]


def thr32(thr):
    """`sim_fp32 >= threshold` compares fp32 numbers: the python threshold is rounded to fp32 first."""
    return float(torch.tensor(float(thr), dtype=torch.float32))


def cubes_of(x):
    """logical [T, C, H, W] -> ([B, side, side, side, C] whole cubes, number of remainder frames)."""
    T, C, H, W = x.shape
    assert H == W and T >= W
    B = T // W
    return x[:B * W].permute(0, 2, 3, 1).reshape(B, W, H, W, C), T - B * W


def pyramid(cubes, root_level):
    """The oracle's pyramid, root level first (every level in the input dtype, one rounding per level)."""
    sizes = OC.side_levels(cubes.shape[1])
    target = sizes[root_level]
    levels = [cubes]
    while levels[0].shape[1] != target:
        levels.insert(0, OC.pool_cube_level(levels[0]))
    return levels


def slot_rows(child):
    """child [B, s, s, s, C] -> ([B, n, n, n, 8, C] the row each parent cell compares in each slot, ok [n, n, n, 8]): slots without
    a child hold child cell (0, 0, 0) of the same cube."""
    s = child.shape[1]
    start, count = OC._child_index(s)
    rows, oks = [], []
    for dt, dy, dx in SLOTS:
        ok = (count[:, None, None] > dt) & (count[None, :, None] > dy) & (count[None, None, :] > dx)
        it = torch.where(count > dt, start + dt, torch.zeros_like(start))
        iy = torch.where(count > dy, start + dy, torch.zeros_like(start))
        ix = torch.where(count > dx, start + dx, torch.zeros_like(start))
        g = child[:, it][:, :, iy][:, :, :, ix]
        alias = child[:, 0, 0, 0][:, None, None, None, :].expand_as(g)
        rows.append(torch.where(ok[None, :, :, :, None], g, alias))
        oks.append(ok)
    return torch.stack(rows, dim=4), torch.stack(oks, dim=3)


def level_sims(parent, child):
    """(sim32, sim64) [B, n, n, n, 8]: the oracle's fp32 cosine and the float64 cosine of the same rows (F.cosine_similarity's
    formula, each norm clamped at 1e-8)."""
    g, _ = slot_rows(child)
    pf = parent.float()[:, :, :, :, None, :]
    gf = g.float()
    sim32 = F.cosine_similarity(pf.expand_as(gf), gf, dim=-1).double()
    pd, gd = pf.double(), gf.double()
    sim64 = (pd * gd).sum(-1) / (pd.norm(dim=-1).clamp_min(O.EPS_SPATIAL) * gd.norm(dim=-1).clamp_min(O.EPS_SPATIAL))
    return sim32, sim64


def traverse(levels, stops):
    """The oracle's top-down sweep with the stop volumes given (stops[l] bool [B, n, n, n] for l < L-1): returns
    (features [N, C], level of every row, first-corner leaf key of every row), ordered by the key."""
    L = len(levels)
    side = levels[-1].shape[1]
    first = [None] * L
    first[L - 1] = torch.arange(side)
    for l in range(L - 2, -1, -1):
        start, _ = OC._child_index(levels[l + 1].shape[1])
        first[l] = first[l + 1][start]
    alive = torch.ones(levels[0].shape[:4], dtype=torch.bool)
    feats, keys, lvls = [], [], []
    for l in range(L):
        stop = stops[l] if l < L - 1 else torch.ones_like(alive)
        b, t, y, xx = (alive & stop).nonzero(as_tuple=True)
        feats.append(levels[l][b, t, y, xx])
        keys.append(((b * side + first[l][t]) * side + first[l][y]) * side + first[l][xx])
        lvls.append(torch.full_like(b, l))
        if l == L - 1:
            break
        split = alive & ~stop
        start, count = OC._child_index(levels[l + 1].shape[1])
        nxt = torch.zeros(levels[l + 1].shape[:4], dtype=torch.bool)
        for dt, dy, dx in SLOTS:
            ok = (count[:, None, None] > dt) & (count[None, :, None] > dy) & (count[None, None, :] > dx)
            b, t, y, xx = (split & ok[None]).nonzero(as_tuple=True)
            nxt[b, start[t] + dt, start[y] + dy, start[xx] + dx] = True
        alive = nxt
    keys = torch.cat(keys)
    order = torch.argsort(keys)
    return torch.cat(feats)[order], torch.cat(lvls)[order], keys[order]


class OctMargins:
    """Every stop decision of the whole cubes of one video: sim32 / sim64 per (level, cell, slot), eps, the decisions inside the
    band, and the traversal decided by float32 (`out32`, what OC.octree_cubes returns) and by float64 (`out64`)."""

    def __init__(self, x, thr, root_level):
        cubes, self.drop = cubes_of(x)
        self.thr, self.level32 = thr, thr32(thr)
        self.levels = pyramid(cubes, root_level)
        L = len(self.levels)
        self.sim32, self.sim64 = [], []
        for l in range(L - 1):
            a, b = level_sims(self.levels[l], self.levels[l + 1])
            self.sim32.append(a)
            self.sim64.append(b)
        diffs = [float((a - b).abs().nan_to_num(0.0).max()) for a, b in zip(self.sim32, self.sim64) if a.numel()]
        self.eps = 2.0 * max(diffs or [0.0])
        self.n_decisions = sum(int(a.numel()) for a in self.sim64)
        self.band = [(s - self.level32).abs() <= self.eps for s in self.sim64]
        self.in_band = sum(int(b.sum()) for b in self.band)
        self.stop32 = [(s >= self.level32).all(-1) for s in self.sim32]
        self.stop64 = [(s >= self.level32).all(-1) for s in self.sim64]

    @functools.cached_property
    def _t32(self):
        return traverse(self.levels, self.stop32)

    @functools.cached_property
    def out64(self):
        return traverse(self.levels, self.stop64)[0]

    out32 = property(lambda self: self._t32[0])
    lvl32 = property(lambda self: self._t32[1])
    key32 = property(lambda self: self._t32[2])

    @property
    def levels_emitting(self):
        return sorted(set(self.lvl32.tolist()))

    def last_cube_has_stopped_inner_cell(self):
        """a node above the leaf level among the rows of the last cube"""
        side = self.levels[-1].shape[1]
        B = self.levels[-1].shape[0]
        last = self.key32 >= (B - 1) * side ** 3
        return bool((self.lvl32[last] < len(self.levels) - 1).any())


def check_rows(out, exp, what):
    """The feature bars: NaN / +-Inf at identical positions; fp32 within FP32_TOL * max(1, |exp|); 16-bit rows bit-equal (the pooling
    arithmetic is the oracle's, one rounding per level -- tests/test_hip_octree.py asserts the same)."""
    out, exp = out.cpu(), exp.cpu()
    assert out.dtype == exp.dtype and out.shape == exp.shape, f"{what}: {tuple(out.shape)} {out.dtype}, expected {tuple(exp.shape)} {exp.dtype}"
    if out.dtype != torch.float32:
        assert D.bits_equal_nan_aware(out, exp), f"{what}: 16-bit rows are not bit-equal to the oracle"
        return
    D.check_features_nan_aware(out, exp, what, tol=D.FP32_TOL)


# ----------------------------------------------------------------------------------------------
# even-side ladders
# ----------------------------------------------------------------------------------------------

def _block_ladder(g, shape, C, thr):
    """[*shape, 2, 2, 2, C] float64 blocks (u + s v, 7 x (u - s/7 v)) with v perpendicular to u, |v| = |u| and
    s = sqrt(1 / (thr + delta)^2 - 1): the block mean is u, one cell has cosine thr + delta with it, the other seven are far above.
    Returns (blocks, delta [*shape])."""
    u = D._rand64(g, *shape, C)
    v = D._perp_same_norm(u, g)
    delta = D._rung_table(g, *shape)
    s = torch.sqrt(1.0 / (thr + delta) ** 2 - 1.0)[..., None]
    odd = torch.randint(0, 8, shape, generator=g)
    blk = torch.empty(*shape, 2, 2, 2, C, dtype=torch.float64)
    for k, (dt, dy, dx) in enumerate(SLOTS):
        blk[..., dt, dy, dx, :] = torch.where((odd == k)[..., None], u + s * v, u - s / 7 * v)
    return blk, delta


def _blocks_to_grid(blk):
    """[B, n, n, n, 2, 2, 2, C] -> [B, 2n, 2n, 2n, C]"""
    B, n = blk.shape[0], blk.shape[1]
    return blk.permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(B, 2 * n, 2 * n, 2 * n, blk.shape[-1])


class OctLadder:
    """One ladder video.  kind "leaf": every 2x2x2 leaf block is a ladder block with an independent u, so every level above splits
    and each block either stops (one row: its mean) or gives its eight leaves.  kind "upper" (side 8): every 2x2x2 leaf block is
    constant, so its parent on the side-4 level equals its children up to a few ulp (the sequential fp32 sum of eight equal values
    is not always exact: 3x, 5x, 6x, 7x round) and stops with a cosine of 1 - O(1e-7), far above the thresholds; the ladder blocks
    are 2x2x2 groups of side-4 cells, decided at the side-2 roots."""

    def __init__(self, kind, side, B, C, thr, seed, dtype_name):
        assert side in (4, 8, 16) and (kind == "leaf" or side == 8)
        self.kind, self.side, self.B, self.C, self.thr, self.dtype = kind, side, B, C, thr, D.DTYPES[dtype_name]
        g = torch.Generator().manual_seed(int(seed))
        if kind == "leaf":
            n = side // 2
            blk, self.delta = _block_ladder(g, (B, n, n, n), C, thr)
            grid = _blocks_to_grid(blk)
            self.big = 2                                          # leaves per axis of a ladder block
        else:
            blk, self.delta = _block_ladder(g, (B, 2, 2, 2), C, thr)
            grid = _blocks_to_grid(blk).repeat_interleave(2, 1).repeat_interleave(2, 2).repeat_interleave(2, 3)
            self.big = 4
        mem = grid.to(self.dtype).reshape(B * side, side, side, C)
        self.x = mem.permute(0, 3, 1, 2)                          # [T, C, H, W] view of channels-last memory
        self.m = OctMargins(self.x, thr, 0)
        lv = {s.shape[1]: i for i, s in enumerate(self.m.levels)}
        self.lad_level = lv[side // self.big]                     # the level whose cells decide the ladder blocks
        s64, s32 = self.m.sim64[self.lad_level], self.m.sim32[self.lad_level]
        k = s64.argmin(dim=-1, keepdim=True)                      # the deciding slot: the other seven are far above
        self.sim64, self.sim32 = s64.gather(-1, k)[..., 0], s32.gather(-1, k)[..., 0]
        self.far = float(s64.scatter(-1, k, 9.0).min())
        # eps from the ladder level's comparisons (the band of THESE decisions)
        self.eps = 2.0 * float((s32 - s64).abs().max())
        self.level32 = self.m.level32
        self.want64 = (s64 >= self.level32).all(-1)
        self.want32 = (s32 >= self.level32).all(-1)
        self.outside = (self.sim64 - self.level32).abs() > self.eps
        self.stop_rows = self.m.levels[self.lad_level]            # [B, n, n, n, C] the row of a stopped block
        self.split_rows = self.m.levels[self.lad_level + 1]       # the rows of a split block's eight parts

    def decode(self, out):
        """The device's (or the oracle's) per-block decisions from the rows alone.  Walk the leaves in order with a cursor into the
        output: at a block's first corner the row is the block mean (stopped: the block's other leaves are skipped) or the block's
        first part; the two differ by s * v, far apart.  Every other row must be the part of a split block it stands for.  Returns
        bool [B, n, n, n]; asserts that the row count is the one these decisions give."""
        out = out.detach().cpu()
        assert out.dtype == self.dtype and out.dim() == 2 and out.shape[1] == self.C
        o = out.double().numpy()
        big, half, S = self.big, self.big // 2, self.side
        stop_rows, split_rows = self.stop_rows.double().numpy(), self.split_rows.double().numpy()
        n = S // big
        stop = np.zeros((self.B, n, n, n), dtype=bool)
        tol = D.FP32_TOL if self.dtype == torch.float32 else D.LOWP_TOL

        def close(row, exp):
            return bool((np.abs(row - exp) <= tol * np.maximum(1.0, np.abs(exp))).all())
        cur = 0
        for b in range(self.B):
            for t in range(0, S, half):
                for y in range(0, S, half):
                    for x in range(0, S, half):
                        bt, by, bx = t // big, y // big, x // big
                        if stop[b, bt, by, bx]:
                            continue
                        assert cur < o.shape[0], f"the output ends after {cur} rows, before leaf {(b, t, y, x)}"
                        part = split_rows[b, t // half, y // half, x // half]
                        if t % big == 0 and y % big == 0 and x % big == 0:
                            mean = stop_rows[b, bt, by, bx]
                            is_stop, is_split = close(o[cur], mean), close(o[cur], part)
                            assert is_stop != is_split, f"row {cur} (block {(b, bt, by, bx)}) is {'both' if is_stop else 'neither'} the block mean nor its first part"
                            stop[b, bt, by, bx] = is_stop
                        else:
                            assert close(o[cur], part), f"row {cur} is not part {(b, t, y, x)} of a split block"
                        cur += 1
        assert cur == o.shape[0], f"{o.shape[0]} rows, the decoded decisions account for {cur}"
        want_rows = int(stop.sum()) + 8 * int((~stop).sum())
        assert cur == want_rows
        return torch.from_numpy(stop)

    def assert_outside_band(self, got, what):
        bad = (got != self.want64) & self.outside
        if bool(bad.any()):
            i = tuple(bad.nonzero()[0].tolist())
            raise AssertionError(f"{what}: {int(bad.sum())} of {int(self.outside.sum())} decisions outside the band (eps {self.eps:.2e}) "
                                 f"differ from float64; first at {i}: sim64 - thr = {float(self.sim64[i] - self.level32):+.3e}, got {bool(got[i])}")

    def in_band_by_rung(self):
        return {r: int(((~self.outside) & (self.delta.abs() == r)).sum()) for r in D.RUNGS}


@functools.lru_cache(maxsize=None)
def oct_ladder(kind, side, B, C, thr, seed, dtype_name):
    return OctLadder(kind, side, B, C, thr, seed, dtype_name)


# (kind, side, cubes, C, thr, seed, dtype).  C = 64: eight independent u's have cosine ~ 1/sqrt(8) +- 0.1 with their mean, far below
# the thresholds, so every level above a leaf ladder splits
LADDERS = [
    ("leaf", 4, 24, 64, 0.8, 301, "float32"), ("leaf", 8, 3, 64, 0.8, 302, "float32"), ("leaf", 16, 1, 64, 0.8, 303, "float32"),
    ("leaf", 8, 3, 64, 0.94, 304, "float32"), ("leaf", 8, 3, 256, 0.8, 305, "float32"),
    ("leaf", 8, 3, 64, 0.75, 309, "float32"),              # 0.75 has an even fp32 mantissa, 0.8 and 0.94 odd ones (thr_lo_sq_of's tie rule)
    ("leaf", 8, 3, 64, 0.8, 306, "bfloat16"), ("leaf", 8, 3, 64, 0.8, 307, "float16"), ("leaf", 16, 1, 64, 0.94, 308, "bfloat16"),
    ("upper", 8, 40, 64, 0.8, 311, "float32"), ("upper", 8, 40, 64, 0.94, 312, "float32"), ("upper", 8, 40, 64, 0.8, 313, "bfloat16"),
]


def ladder_id(spec):
    kind, side, B, C, thr, seed, d = spec
    return f"{kind}_s{side}_B{B}_C{C}_{thr}_{D.SHORT[d]}"


# ----------------------------------------------------------------------------------------------
# degenerate clips pinned to the reference (tests/golden/odo_*.npz, made by make_golden_octree_offdist.py)
# ----------------------------------------------------------------------------------------------

DEG_SIDES = {7: 12, 5: 16}                                   # side -> C; two cubes plus a remainder frame
DEG_THR = 0.8


DEG_SPREAD = 0.6


def _deg_base(side):
    """One common token plus DEG_SPREAD times the smooth synth-v1 preset: every cosine of the clip -- the alias comparisons with the
    unrelated origin leaf included -- lies around the ordinary threshold (~ 1 / sqrt((1 + a^2 / 8) (1 + a^2)) = 0.84 for a = 0.6), so
    cells with missing slots stop or split on their alias slots, which an unrelated Gaussian origin never lets them do."""
    C = DEG_SIDES[side]
    x = synth_video(2 * side + 1, C, side, side, seed=20 + side, c=0.15, p_static=0.7)
    common = torch.randn(C, generator=torch.Generator().manual_seed(120 + side))
    x.permute(0, 2, 3, 1).mul_(DEG_SPREAD).add_(common)
    return x


def build_deg(kind, side):
    """[T, C, side, side] float32 view of channels-last memory; T = two cubes plus one remainder frame."""
    x = _deg_base(side)
    m = x.permute(0, 2, 3, 1)
    assert m.is_contiguous()
    S = side
    if kind == "const":
        m[:] = m[0, 0, 0].clone()
    elif kind == "static":
        m[:] = m[0].clone()
    elif kind == "zero_origin":
        m[S, 0, 0] = 0                                       # leaf (0, 0, 0) of the second cube: the alias of its missing slots
    elif kind == "zero_cube":
        m[S:2 * S] = 0
    elif kind == "zero_video":
        m.zero_()
    elif kind == "nan_origin":
        m[0, 0, 0, 3] = float("nan")                         # poisons every alias comparison of the first cube
    elif kind == "nan_inner":
        m[S + 2, 3, 1, 5] = float("nan")
    elif kind == "inf_origin":
        m[S, 0, 0, 2] = float("inf")
    elif kind == "pm_inf":
        m[3, 2, 4, 1] = float("-inf")
        m[3, 2, 4, 6] = float("inf")
    elif kind == "scale_p62":
        m.mul_(2.0 ** 62)
    elif kind == "scale_m70":
        m.mul_(2.0 ** -70)
    else:
        raise ValueError(kind)
    return x


DEG_KINDS = ("const", "static", "zero_origin", "zero_cube", "zero_video", "nan_origin", "nan_inner", "inf_origin", "pm_inf", "scale_p62",
             "scale_m70")
# the subset that also runs at the edge thresholds
DEG_EDGE_KINDS = ("const", "static", "zero_origin", "zero_video", "nan_origin", "inf_origin", "scale_m70")
DEG_EDGE_THRS = (0.0, -0.3, 1.0, 1.5)


def deg_thresholds(kind):
    return (DEG_THR,) + (DEG_EDGE_THRS if kind in DEG_EDGE_KINDS else ())


def deg_cases():
    """[(kind, side, thr)]"""
    return [(k, s, t) for s in DEG_SIDES for k in DEG_KINDS for t in deg_thresholds(k)]


def deg_file(kind, side):
    return f"odo_{kind}_s{side}"


def deg_id(case):
    kind, side, thr = case
    return f"{deg_file(kind, side)}_{thr}"


@functools.lru_cache(maxsize=None)
def _deg_npz(kind, side):
    z = np.load(os.path.join(GOLDEN_DIR, deg_file(kind, side) + ".npz"))
    return {k: z[k] for k in z.files}


def load_deg(case):
    """One (kind, side, threshold) of tests/golden/odo_<kind>_s<side>.npz -> (x [T, C, side, side], the reference's features)."""
    kind, side, thr = case
    z = _deg_npz(kind, side)
    meta = json.loads(str(z["meta"]))
    i = meta["thresholds"].index(thr)
    return _t(z["x_thwc"], "float32").permute(0, 3, 1, 2), _t(z[f"feat{i}"], "float32")


def is_const_thr1(case):
    """A constant video at threshold 1.0: sim64 is 1 up to rounding, every decision is in the band by construction and the
    reference's own fp32 rounding decides it.  No row count is pinned there.  (The pooled means of a constant token are NOT all
    bit-equal to it -- the reference's own rows are up to 3 ulp off, a sequential fp32 sum of equal values rounds at 3x, 5x, ... --
    so the rows are held to the pyramid's cells bit for bit, and to the token within the feature bar.)"""
    return case[0] == "const" and case[2] == 1.0


class DegExpect:
    """What a degenerate clip pins.

    `pinned`: the reference's rows, exactly.  Every decision is outside the band, or inside it with a similarity of exactly 0 (zero
    rows: 0 in any summation order), or the clip is scale_p62, whose fp32 norms overflow in any order (sim32 is 0 where sim64 is not:
    the margin says nothing there), or -- threshold 1.0 on clips with bit-identical parent and child rows, sim64 = 1 up to rounding --
    the in-band slots sit in cells that another slot fails anyway: the traversal with every in-band slot passing (`n_min` rows, the
    fewest) and with every one failing (`n_max` rows, the most) coincide, so the result is determined.

    Otherwise the reference's fp32 rounding decides the `open_cells` (cells that stop with every in-band slot passing and split with
    every one failing) and no row count is pinned.  With few open cells (the static clips) `check_open` asks for an assignment of
    them whose traversal reproduces the rows exactly, in order: every other decision and the emission order are the float64
    traversal's.  With many (the constant clips: every cell is open, and all rows are the same token up to a few ulp, so order and
    cell identity are not observable) `check_free` bounds the count and holds every row to a cell of the pyramid (`cells`)."""

    MAX_OPEN = 12

    def __init__(self, case):
        kind, side, thr = case
        x, self.feat = load_deg(case)
        self.x, self.T, self.side = x, x.shape[0], side
        m = OctMargins(x, thr, 0)
        self.m = m
        free = [b & (s != 0.0) for s, b in zip(m.sim64, m.band)]
        self.in_band = sum(int(f.sum()) for f in free)
        self.pinned = kind == "scale_p62" or self.in_band == 0
        self.n_open = 0
        if not self.pinned:
            self.stop_hi = [((s >= m.level32) | b).all(-1) for s, b in zip(m.sim64, m.band)]
            self.stop_lo = [((s >= m.level32) & ~b).all(-1) for s, b in zip(m.sim64, m.band)]
            self.n_min, self.n_max = traverse(m.levels, self.stop_hi)[0].shape[0], traverse(m.levels, self.stop_lo)[0].shape[0]
            self.open_cells = [(l, tuple(i.tolist())) for l, (h, lo) in enumerate(zip(self.stop_hi, self.stop_lo)) for i in (h != lo).nonzero()]
            self.n_open = len(self.open_cells)
            self.cells = torch.cat([lv.reshape(-1, lv.shape[-1]) for lv in m.levels])
            self.pinned = self.n_min == self.n_max
        self.enumerable = not self.pinned and self.n_open <= self.MAX_OPEN

    def rows_are_cells_bitwise(self, cube_rows):
        """every row is bit-equal to a cell of the oracle's pyramid (the device pools in the oracle's order); float32 rows only"""
        assert cube_rows.dtype == torch.float32 and self.cells.dtype == torch.float32
        have = {bytes(r) for r in self.cells.contiguous().view(torch.int32).numpy().view(np.uint8).reshape(self.cells.shape[0], -1)}
        rows = cube_rows.cpu().contiguous().view(torch.int32).numpy().view(np.uint8).reshape(cube_rows.shape[0], -1)
        return all(bytes(r) in have for r in rows)

    def check_open(self, cube_rows, what):
        """Some assignment of the open cells reproduces the rows exactly (count, order, NaN / Inf pattern, finite values within the
        feature bar).  Returns the number of open cells that stopped."""
        assert self.enumerable
        cube_rows = cube_rows.cpu()
        assert self.n_min <= cube_rows.shape[0] <= self.n_max, f"{what}: {cube_rows.shape[0]} cube rows, outside [{self.n_min}, {self.n_max}]"
        for mask in range(1 << self.n_open):
            stops = [s.clone() for s in self.stop_lo]
            for k, (l, idx) in enumerate(self.open_cells):
                if mask >> k & 1:
                    stops[l][idx] = True
            exp = traverse(self.m.levels, stops)[0]
            if exp.shape != cube_rows.shape:
                continue
            try:
                D.check_features_nan_aware(cube_rows, exp, what, tol=D.FP32_TOL)
            except AssertionError:
                continue
            return bin(mask).count("1")
        raise AssertionError(f"{what}: no assignment of the {self.n_open} in-band cells gives these rows in this order")

    def check_free(self, cube_rows, what):
        cube_rows = cube_rows.cpu()
        n = cube_rows.shape[0]
        assert self.n_min <= n <= self.n_max, f"{what}: {n} cube rows, outside [{self.n_min}, {self.n_max}]"
        fin = torch.isfinite(cube_rows).all(-1)
        cells = self.cells[torch.isfinite(self.cells).all(-1)].double()
        rows = cube_rows[fin].double()
        d = (rows[:, None, :] - cells[None, :, :]).abs() / cells[None, :, :].abs().clamp_min(1.0)
        worst = float(d.max(-1).values.min(-1).values.max()) if rows.numel() else 0.0
        assert worst <= D.FP32_TOL, f"{what}: a row is no cell of the pyramid (distance {worst:.2e})"
        assert int((~fin).sum()) <= int((~torch.isfinite(self.cells).all(-1)).sum())
        return n


@functools.lru_cache(maxsize=None)
def deg_expect(case):
    return DegExpect(case)


def root_count(T, side, root_level=0):
    """rows when every root stops: the root cells of the whole cubes plus the quadtree roots of the remainder frames"""
    n = OC.side_levels(side)[root_level]
    return (T // side) * n ** 3 + (T % side) * n * n


# ----------------------------------------------------------------------------------------------
# dispatch and shape edges against the oracle
# ----------------------------------------------------------------------------------------------

def make_video(kind, T, C, side, seed, dtype):
    if kind == "synth":
        return synth_video(T, C, side, side, seed=seed, dtype=dtype)
    if kind == "smooth":
        return synth_video(T, C, side, side, seed=seed, dtype=dtype, c=0.15, p_static=0.7)
    if kind == "iid":
        return iid_video(T, C, side, side, seed=seed, dtype=dtype)
    if kind == "heavy":
        return heavy_video(T, C, side, side, seed=seed, n_massive=2, scale=30.0, dtype=dtype)
    raise ValueError(kind)


class Case:
    """One video of the dispatch table with its margins and the oracle's result."""

    def __init__(self, kind, T, C, side, dtype_name, thr, root, seed):
        self.spec = (kind, T, C, side, dtype_name, thr, root, seed)
        self.thr, self.root = thr, root
        self.x = make_video(kind, T, C, side, seed, D.DTYPES[dtype_name])
        self.m = OctMargins(self.x, thr, root)
        self.exp = OC.get_octree_features(self.x, thr, root)
        self.rem_in_band = 0
        if self.m.drop:                                      # the remainder frames go through the spatial quadtree
            rm = D.Margins(self.x[T - self.m.drop:], thr, -1.0, root)
            self.rem_in_band = int(rm.band_boxes.shape[0])


@functools.lru_cache(maxsize=None)
def _case(kind, T, C, side, dtype_name, thr, root, seed):
    return Case(kind, T, C, side, dtype_name, thr, root, seed)


def case(kind, T, C, side, dtype_name, thr, root, seed):
    """(a negative root_level names the same pyramid as its non-negative twin: one Case for both)"""
    n = len(OC.side_levels(side))
    return _case(kind, T, C, side, dtype_name, thr, root + n if -n <= root < 0 else root, seed)


def case_id(spec):
    kind, T, C, side, d, thr, root, seed = spec
    return f"{kind}_T{T}_C{C}_s{side}_{D.SHORT[d]}_{thr}_r{root}"


# pack widths: float32 C = 7 / 6 / 12 run scalar / 2-wide / 4-wide packs, 16-bit C = 6 / 12 / 24 run packs of 2 / 4 / 8
PACK_CASES = [("smooth", 10, 7, 5, "float32", 0.8, 0, 1), ("smooth", 10, 6, 5, "float32", 0.8, 0, 2), ("smooth", 10, 12, 5, "float32", 0.8, 0, 3)]
PACK_CASES += [("smooth", 10, c, 5, d, 0.8, 0, 4 + i) for d in ("bfloat16", "float16") for i, c in enumerate((6, 12, 24))]
# row tails: fp32 C = 1100 is four full 256-channel iterations of the stop loop plus 76; bf16 C = 520 is one full 512-channel
# iteration plus 8; bf16 C = 3584 (one cube of side 7) is 2048 + 1536 in the gather's four-chunk loop
TAIL_CASES = [("smooth", 5, 1100, 5, "float32", 0.8, 0, 11), ("smooth", 5, 520, 5, "bfloat16", 0.8, 0, 12),
              ("smooth", 7, 3584, 7, "bfloat16", 0.8, 0, 13)]
SIDES = (2, 3, 4, 5, 9, 16, 17, 33)
SIDE_THR = {4: 0.6}                    # at 0.8 no root of the side-4 clips stops (one level only); the others run at 0.8


def side_cases():
    """every valid root_level of every side, non-negative and negative, C = 8"""
    out = []
    for side in SIDES:
        n = len(OC.side_levels(side))
        T = 2 * side if side <= 9 else side
        for r in list(range(n)) + list(range(-n, 0)):
            out.append(("smooth", T, 8, side, "float32", SIDE_THR.get(side, 0.8), r, 40 + side))
    return out


SIDE_CASES = side_cases()
# scan boundaries: side 16 is exactly 4096 leaves (one scan workgroup) per cube; 1, 2, 3 cubes plus one remainder frame
SCAN_CASES = [("smooth", 16 * k + 1, 8, 16, "float32", thr, 0, 60 + k) for k in (1, 2, 3) for thr in (0.8, 2.0, -2.0)]
# grid-stride: 766 cubes of side 14 at root_level 1 (4-7-14): the side-7 level has 766 * 343 = 262 738 cells, more than the 262 144
# waves of a full k_oct_stop launch, and the 2.1 M leaves wrap k_oct_gather's loop eight times; 3 remainder frames
GRID_CASE = ("smooth", 766 * 14 + 3, 2, 14, "float32", 0.8, 1, 70)
WS_BIG = ("smooth", 48, 8, 16, "float32", 0.8, 0, 80)
WS_SMALL = ("smooth", 5, 8, 5, "float32", 0.8, 0, 81)
ORDINARY = PACK_CASES + TAIL_CASES + SIDE_CASES + [c for c in SCAN_CASES if abs(c[5]) < 1.5] + [WS_BIG, WS_SMALL]
