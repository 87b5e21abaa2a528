"""Cases and references for the three consumers of a finished quadtree merge's tables (meta, lab_row, gcnt, frame_cnt, rc_list, cgeo,
the node rows S): `pos_embs=` pooling (sttm_quadtree_apply), the token map (sttm_quadtree_token_map) and the merged tokens' 1-d indices
(`return_idx=True`).  Shared by tests/test_consumers_cpu.py and tests/test_hip_consumers.py; everything here runs on the CPU.

References.
  * the oracle with `pos_embs=(coord, rnd)`: referee of the pooled rows in both modes;
  * `tests/_token_map_ref.ref_token_maps`: referee of the maps;
  * the float64 centroid: in weighted mode (`pos_emb_weighted_avg=True`) the pooled row of output r is the mean of the side tensor over
    the tokens whose token_to_out == r (sum-pooled pyramid, summed over the group, divided by the group's patch count:
    quadtree_builder.py:75-81, quadtree_temporal_merger.py:153-169).  It is computed by scatter-add from the map alone, so it does not
    go through the oracle's pyramid code, and it ties the apply path to the map.

Side tensors.  `coord` carries the channels (t, y, x, 1, t*H*W + y*W + x, 0 ...): its centroid is a group's centre of mass, its ones
channel pools to exactly 1 (a sum of ones equal to the patch count, divided by the patch count: 1 exactly if and only if the
accumulated sum IS the patch count), and every value is a small integer the side dtype holds or rounds once at construction.  `rnd`
is uniform in [-1, 1) like a RoPE cos / sin table: values of O(1), compared with the oracle on the project's absolute bars.

Decisive cases.  A device sum and the reference sum may err in opposite directions, so a similarity closer to its threshold than
eps = 2 * max |sim_oracle_fp32 - sim_float64| (tests/_offdist.py) may legitimately be decided differently; every case used here keeps
all its spatial and temporal similarities outside that band (`band(...)`; the CPU test asserts it for every case), so index-exact
comparisons with the oracle are owed by every producer path.  NaN similarities (NaN / Inf clips) compare false with every threshold
in every arithmetic: they are outside the band as long as the fp32 and the float64 value are both NaN.
"""
import functools

import torch

from oracle import sttm_oracle as O
from sttm_amd.synth import synth_video
from tests import _offdist as D
from tests._token_map_ref import ref_token_maps

# ----------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------

# name -> (T, C, H, W, dtype, threshold, temporal_thresh, root_level, seed, side width Cv)
SHAPES = {
    "A": (12, 64, 14, 14, "float32", 0.85, 0.55, 1, 700, 16),        # 3-level tree: every label path, the column walk
    "A16": (12, 128, 14, 14, "bfloat16", 0.85, 0.55, 1, 701, 16),
    "B": (2, 16, 64, 64, "float32", 0.85, 0.55, 0, 702, 8),          # 6 levels, four scan chunks, the whole-workgroup tail of idx_out
    "C": (3, 16, 34, 40, "float32", 0.85, 0.55, 1, 703, 8),          # 5 levels, two scan chunks; 17 x 20 is mixed parity: map and index only
    "C2": (3, 16, 40, 40, "float32", 0.85, 0.55, 1, 707, 8),         # ... the same depth and chunk count on a grid pos_embs accepts
    "D": (8, 1024, 14, 14, "float32", 0.85, 0.55, 2, 704, 32),       # the channel-tiled producer under wide_lanes=256
    "E": (8, 64, 13, 24, "float32", 0.85, 0.60, 1, 705, 16),         # alias cells; mixed parity: map and index only
    # 6 levels with groups of 12 members: the group mean hands groups of more than 10 members to the whole workgroup, and only root
    # cells of more than 64 leaves have that tail -- B's two frames never reach it.  Frames 0-11 are one frame repeated, frame 12 is
    # unrelated (groups of one and two members beside the long ones).
    "F": (13, 16, 40, 40, "float32", 0.85, 0.55, 0, 708, 8),
}


def _static_then_one(T, C, H, W, seed, dtype):
    a = synth_video(1, C, H, W, seed=seed, dtype=dtype).permute(0, 2, 3, 1)
    b = synth_video(1, C, H, W, seed=seed + 50, dtype=dtype).permute(0, 2, 3, 1)
    return torch.cat([a.expand(T - 1, -1, -1, -1), b]).contiguous().permute(0, 3, 1, 2)


BUILDERS = {"F": _static_then_one}
MIXED_PARITY = ("C", "E")                                            # pos_embs and weighted_avg are refused (reference: RuntimeError)
# call flags that change the result (each gets its own reference); temporal_thresh=-1 switches the temporal stage off
FLAGS = {"plain": {}, "slow": dict(slow_ver=True), "head16": dict(head_dim=16), "weighted": dict(weighted_avg=True),
         "spatial": dict(temporal_thresh=-1.0)}
# side tensors that differ from the bf16 C=128 features (256-byte rows) in dtype and width: name -> (dtype, Cv)
SIDE_VARIANTS = {"f32_Cv32": ("float32", 32), "bf16_Cv16": ("bfloat16", 16), "f32_Cv6": ("float32", 6)}
SIDE_TOO_WIDE = ("float32", 128)                                     # 512-byte side rows on 256-byte feature rows
OD_CLIPS = ["od_static_f32", "od_dup_frames_f32", "od_allmerge_f32", "od_allmerge_w_f32", "od_zero_frame_f32", "od_const_f32",
            "od_nan_elem_f32", "od_inf_elem_f32", "od_static_bf16", "od_allmerge_bf16"]
OD_EVERY_PATH = OD_CLIPS[:4]


class Case:
    """One input with its call arguments and the side tensors that ride along.  `pos`: "both" (pos_embs accepted in both modes),
    "weighted" (the unweighted mode raises the reference's UnboundLocalError: temporal stage off) or None (mixed parity)."""

    def __init__(self, name, build, dtype, thr, kw, Cv, side_dtype=None, pos="both"):
        self.name, self._build, self.dtype, self.thr, self.kw, self.Cv = name, build, D.DTYPES[dtype], thr, dict(kw), Cv
        self.side_dtype = D.DTYPES[side_dtype] if side_dtype else self.dtype
        self.pos = pos

    @functools.cached_property
    def x(self):
        return self._build()

    @property
    def args(self):
        """(threshold, temporal_thresh, root_level, weighted_avg, slow_ver, head_dim) for ref_token_maps."""
        k = self.kw
        return (self.thr, k.get("temporal_thresh", -1.0), k.get("root_level", 0), k.get("weighted_avg", False), k.get("slow_ver", False),
                k.get("head_dim"))

    def __repr__(self):
        return self.name


def _synth_case(shape, flag):
    T, C, H, W, dname, thr, tthr, root, seed, Cv = SHAPES[shape]
    kw = dict(temporal_thresh=tthr, root_level=root)
    kw.update(FLAGS[flag])
    pos = None if shape in MIXED_PARITY else ("weighted" if kw["temporal_thresh"] <= 0 else "both")
    build = BUILDERS.get(shape, lambda T, C, H, W, seed, dtype: synth_video(T, C, H, W, seed=seed, dtype=dtype))
    return Case(f"{shape}-{flag}", lambda: build(T, C, H, W, seed, D.DTYPES[dname]), dname, thr, kw, Cv, pos=pos)


def _od_case(fid):
    c = D.load_od(fid)
    thr, kw = D.od_kwargs(c["meta"])
    return Case(fid, lambda: c["x"], c["meta"]["dtype"], thr, kw, 16)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case: every input of tests/test_hip_consumers.py."""
    out = {}
    for shape in SHAPES:
        for flag in FLAGS:
            if shape in MIXED_PARITY and flag == "weighted":
                continue                        # sum pooling on mixed parity: refused (tests/test_hip_consumers.py asserts the error)
            c = _synth_case(shape, flag)
            out[c.name] = c
    T, C, H, W, dname, thr, tthr, root, seed, _ = SHAPES["A16"]
    for vname, (sd, cv) in SIDE_VARIANTS.items():
        out[f"A16-{vname}"] = Case(f"A16-{vname}", lambda: synth_video(T, C, H, W, seed=seed, dtype=D.DTYPES[dname]), dname, thr,
                                   dict(temporal_thresh=tthr, root_level=root), cv, side_dtype=sd)
    for fid in OD_CLIPS:
        out[fid] = _od_case(fid)
    out["allmerge_T128"] = Case("allmerge_T128", lambda: D.allmerge_video(128, torch.float32), "float32", 0.85,
                                dict(temporal_thresh=0.55, root_level=1), 16)
    out["one_frame"] = Case("one_frame", lambda: synth_video(1, 64, 14, 14, seed=706), "float32", 0.85, dict(temporal_thresh=0.55, root_level=1), 16)
    return out


def case_names(pos_only=False):
    return [n for n, c in cases().items() if c.pos or not pos_only]


# ----------------------------------------------------------------------------------------------
# side tensors and references
# ----------------------------------------------------------------------------------------------

ONES, FLAT = 3, 4                                # channels of `coord`


def side_tensors(T, H, W, Cv, dtype, seed=0):
    """(coord, rnd): logical [T, Cv, H, W] views of dense [T, H, W, Cv] memory."""
    assert Cv >= 5
    t, y, x = torch.meshgrid(torch.arange(T), torch.arange(H), torch.arange(W), indexing="ij")
    coord = torch.zeros(T, H, W, Cv, dtype=torch.float64)
    for k, v in enumerate((t, y, x, torch.ones_like(t), (t * H + y) * W + x)):
        coord[..., k] = v
    g = torch.Generator().manual_seed(9000 + seed)
    rnd = torch.rand(T, H, W, Cv, generator=g) * 2 - 1
    return coord.to(dtype).permute(0, 3, 1, 2), rnd.to(dtype).permute(0, 3, 1, 2)


def centroid64(side, token_to_out, n_out):
    """float64 mean of `side` ([T, Cv, H, W]) over the tokens of every output row."""
    rows = side.permute(0, 2, 3, 1).reshape(-1, side.shape[1]).double()
    idx = token_to_out.reshape(-1).long()
    acc = torch.zeros(n_out, rows.shape[1], dtype=torch.float64).index_add_(0, idx, rows)
    return acc / torch.bincount(idx, minlength=n_out).double()[:, None]


def deviation(rows, c64):
    """max |rows - c64| / max(1, |c64|): the measure of every centroid comparison."""
    return float(((rows.double() - c64).abs() / c64.abs().clamp_min(1.0)).max())


def rounding_bound(c):
    """What the oracle's own arithmetic can lose against the float64 centroid, from the number formats alone: every term is >= 0, so a
    chain of k additions / one division in a format of unit roundoff u stays within (k + 1) u of the exact value, relatively.  A
    token's value passes 3 additions per pyramid level and one per node of its group before the division; finfo.eps = 2 u."""
    ref = reference(c.name)
    members = int(torch.bincount(ref["maps"]["out_of_node"]).max())
    levels = O.Geometry(c.x.shape[2], c.x.shape[3], c.kw.get("root_level", 0)).n_level
    return (3 * levels + members + 1) * torch.finfo(c.side_dtype).eps


@functools.lru_cache(maxsize=None)
def reference(name):
    """Computed once per case and left unchanged: maps (ref_token_maps), the side tensors, the oracle's pooled rows in both modes
    (None where the reference raises) and the float64 centroids of both side tensors."""
    c = cases()[name]
    T, _, H, W = c.x.shape
    maps = ref_token_maps(c.x, *c.args)
    out = dict(maps=maps)
    if c.pos:
        pe = side_tensors(T, H, W, c.Cv, c.side_dtype)
        kw = dict(c.kw)
        out["pe"] = pe
        for mode, key in ((False, "pos_u"), (True, "pos_w")):
            if mode or c.pos == "both":
                r = O.get_quadtree_features(c.x, c.thr, pos_embs=pe, pos_emb_weighted_avg=mode, **kw)
                assert torch.equal(r[2], maps["tlbr"]) and torch.equal(r[1], maps["npatch"])
                out[key] = r[3]
        n = maps["tlbr"].shape[0]
        out["centroid"] = tuple(centroid64(p, maps["token_to_out"], n) for p in pe)
    return out


@functools.lru_cache(maxsize=None)
def oracle_deviation(side_dtype):
    """The oracle's own largest deviation from the float64 centroid over every case whose side tensors have this dtype (weighted mode,
    both side tensors).  Twice this is the bar of the device's rows: its summation order differs from the oracle's and both round in
    fp32 or in the side dtype."""
    worst = 0.0
    for name in case_names(pos_only=True):
        if cases()[name].side_dtype == side_dtype:
            ref = reference(name)
            worst = max([worst] + [deviation(p, c64) for p, c64 in zip(ref["pos_w"], ref["centroid"])])
    return worst


# ----------------------------------------------------------------------------------------------
# decisiveness
# ----------------------------------------------------------------------------------------------

class band:
    """Every similarity the oracle compares with a threshold on one case, next to the float64 similarity of the same rows;
    eps_* = 2 * max |sim_fp32 - sim_float64| per stage (tests/_offdist.py); `in_band` counts the decisions that a different summation
    order could flip: a spatial parent unless all four slots are more than eps above the threshold or one is more than eps below it or
    NaN, a candidate pair unless it is more than eps from the temporal threshold or NaN.  slow_ver thresholds the same candidate
    pairs on the whole-vector similarity (quadtree_temporal_merger.py:75-121), so its pairs are measured on the fast filter's list."""

    def __init__(self, c):
        thr, tthr, root, weighted, slow, head = c.args
        sp, tp = [], []
        cos32, keep32 = O._cosine, O.keep_similar_pairs

        def cosine(p, ch, hd):
            s32 = cos32(p, ch, hd)
            sp.append((s32.double(), D._cos64(p.double(), ch.double(), hd)))
            return s32

        def keep(rows, pairs, tt, hd=None):
            hd = None if slow else hd
            s32 = O.pair_similarity(O.unit_rows(rows, hd), pairs)
            d = rows.double()
            if hd is not None:
                d = d.reshape(d.shape[0], -1, hd)
            dn = d / (d.norm(dim=-1, keepdim=True) + O.EPS_TEMPORAL)
            s = (dn[pairs[:, 0]] * dn[pairs[:, 1]]).sum(-1)
            tp.append((s32.double(), s.mean(-1) if s.dim() == 2 else s))
            return pairs[s32 >= tt]

        O._cosine, O.keep_similar_pairs = cosine, keep
        try:
            O.get_quadtree_features(c.x, thr, tthr, root, weighted, False, False, head)
        finally:
            O._cosine, O.keep_similar_pairs = cos32, keep32
        thr32 = float(torch.tensor(thr, dtype=torch.float32))
        tthr32 = float(torch.tensor(tthr, dtype=torch.float32))
        self.eps_sp, self.eps_tp = self._eps(sp), self._eps(tp)
        self.n_decisions = self.in_band = self.nan_mismatch = 0
        for s32, s64 in sp:
            nan = torch.isnan(s64)
            self.nan_mismatch += int((nan != torch.isnan(s32)).sum())
            clear = (((s64 - thr32) > self.eps_sp).all(-1) | ((thr32 - s64) > self.eps_sp).any(-1) | nan.any(-1))
            self.n_decisions += clear.numel()
            self.in_band += int((~clear).sum())
        for s32, s64 in tp:
            nan = torch.isnan(s64)
            self.nan_mismatch += int((nan != torch.isnan(s32)).sum())
            clear = ((s64 - tthr32).abs() > self.eps_tp) | nan
            self.n_decisions += clear.numel()
            self.in_band += int((~clear).sum())
        self.decisive = self.in_band == 0 and self.nan_mismatch == 0

    @staticmethod
    def _eps(pairs):
        worst = 0.0
        for a, b in pairs:
            d = (a - b).abs()
            d = d[torch.isfinite(d)]
            if d.numel():
                worst = max(worst, float(d.max()))
        return 2.0 * worst


# ----------------------------------------------------------------------------------------------
# producer settings
# ----------------------------------------------------------------------------------------------

def producer_settings(shape):
    """The sttm_configure settings that select another producer of the tables (or another work split of the group mean) without
    changing a result; the default setting is not in the list."""
    from tests.test_hip_parity import LABEL_PATHS
    s = [dict(p) for p in LABEL_PATHS if p]
    s += [dict(col_walk=2), dict(col_walk=2, col_frames=3, col_cap=2), dict(gm_split=1), dict(gm_split=64)]
    if shape in ("B", "C", "C2", "F"):                        # trees of 4 and more levels: the one-workgroup form instead of the split form
        s += [dict(k1_split=-1), dict(k1_split=-1, gm_split=1)]
    if shape == "D":
        s += [dict(wide_lanes=256), dict(wide_lanes=256, no_fuse=1), dict(wide_lanes=256, fold_labels=1), dict(wide_lanes=256, gm_split=1)]
    return s


def setting_id(opts):
    return "+".join(f"{k}={v}" for k, v in opts.items()) or "default"


class configured:
    """sttm_configure switches for the duration of a block: the context manager of tests/test_hip_offdist.py (which restores the label,
    column-walk and k1_split knobs) plus the two knobs only this file turns, gm_split and wide_lanes.  Every knob is restored, also when
    the block, or setting a knob, raised."""

    def __init__(self, **opts):
        from tests.test_hip_offdist import _configured
        self.inner = _configured(**opts)

    def __enter__(self):
        try:
            self.inner.__enter__()
        except BaseException:
            self.__exit__(None, None, None)
            raise

    def __exit__(self, *exc):
        from sttm_amd import _lib
        try:
            self.inner.__exit__(*exc)
        finally:
            _lib.configure(gm_split=0, wide_lanes=0)
