"""GPU: the three consumers of a finished merge's tables -- `pos_embs=` pooling (sttm_quadtree_apply), the token map
(sttm_quadtree_token_map; vis_flag=True, unmerge_tokens) and the merged tokens' 1-d indices (`return_idx=True`) -- behind every
producer of those tables: the label paths, the column walk, the split / one-workgroup / channel-tiled spatial stages, the work splits
of the group mean, slow_ver / head_dim / weighted_avg, the identity labels of a call without the temporal stage, and the
off-distribution clips of tests/_offdist.py.  Cases and references: tests/_consumers.py (checked by tests/test_consumers_cpu.py).

On the default setting everything is compared with the references; every other setting must reproduce the default setting's bits
("none of them changes results").  Measured figures: profiles/consumers_on_every_path.md.
"""
import pytest
import torch

from tests import _consumers as C
from tests import _offdist as D

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _tol(dtype):
    from tests.test_hip_parity import BF16_TOL, FP32_TOL
    return FP32_TOL if dtype == torch.float32 else BF16_TOL


def _worst(got, exp):
    """The measure of tests/test_hip_parity.py::_check: absolute for fp32, relative to max(1, |expected|) for 16-bit rows."""
    err = (got.float() - exp.float()).abs()
    scale = exp.float().abs().clamp_min(1.0) if got.dtype != torch.float32 else 1.0
    return float((err / scale).max()) if err.numel() else 0.0


def _worst_rel(got, exp):
    """... relative to max(1, |expected|) in every dtype (tests/_offdist.py): for the coordinate rows, whose values reach 10^4."""
    err = (got.double() - exp.double()).abs() / exp.double().abs().clamp_min(1.0)
    return float(err.max()) if err.numel() else 0.0


def _run(c, xd, ped, want_vis=False):
    """Every consumer once on the current setting: {name: CPU tensor}."""
    import sttm_amd
    from sttm_amd.quadtree_interface import get_quadtree_features_into
    out = {}
    if c.pos:
        for mode, tag in ((False, "u"), (True, "w")):
            if mode or c.pos == "both":
                r = sttm_amd.get_quadtree_features(xd, c.thr, pos_embs=ped, pos_emb_weighted_avg=mode, **c.kw)
                assert len(r) == 4 and len(r[3]) == 2
                out.update({f"feat_{tag}": r[0], f"npatch_{tag}": r[1], f"tlbr_{tag}": r[2], f"coord_{tag}": r[3][0], f"rnd_{tag}": r[3][1]})
    r = sttm_amd.get_quadtree_features_with_map(xd, c.thr, **c.kw)
    out.update(feat=r[0], npatch=r[1], tlbr=r[2], t2o=r[3], t2n=r[4])
    T, Cf, H, W = xd.shape
    dest = torch.empty((T * H * W, Cf), dtype=xd.dtype, device=xd.device)
    r = get_quadtree_features_into(dest, xd, c.thr, return_idx=True, **c.kw)
    out.update(feat_i=r[0], npatch_i=r[1], tlbr_i=r[2], idx=r[3])
    if want_vis:
        r = sttm_amd.get_quadtree_features(xd, c.thr, c.kw["temporal_thresh"], c.kw["root_level"], c.kw.get("weighted_avg", False), True)
        out.update(feat_v=r[0], npatch_v=r[1], tlbr_v=r[2])
        out["node_metadata"] = r[3]
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()}


def _same_bits(out, base, what):
    assert out.keys() == base.keys()
    for k, v in out.items():
        b = base[k]
        if not torch.is_tensor(v):
            assert v == b and list(v) == list(b), f"{what}: {k} differs from the default setting's"
            continue
        assert v.shape == b.shape and v.dtype == b.dtype, f"{what}: {k} has shape {tuple(v.shape)}, the default setting gave {tuple(b.shape)}"
        if not torch.equal(v.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)):
            bad = (v.contiguous().view(torch.uint8) != b.contiguous().view(torch.uint8)).reshape(v.shape[0], -1).any(1).nonzero().flatten()
            raise AssertionError(f"{what}: {k} differs from the default setting's bits in {bad.numel()} rows, first {bad[:5].tolist()}")


def _check_default(c, out, what, feats_exp=None):
    """(a): everything the default setting returns, against the references."""
    ref = C.reference(c.name)
    maps = ref["maps"]
    T, _, H, W = c.x.shape
    exp = feats_exp if feats_exp is not None else (maps["feat"], maps["npatch"], maps["tlbr"])
    D.check_nan_aware((out["feat"], out["npatch"], out["tlbr"]), exp, what)
    if feats_exp is None:                                     # synth-v1 cases: the absolute fp32 bar of tests/test_hip_parity.py
        worst = _worst(out["feat"], exp[0])
        assert worst <= _tol(c.dtype), f"{what}: features {worst:.3e}"
    for tag in ("u", "w", "i", "v"):                          # one merge, whichever consumer rode along
        if f"feat_{tag}" in out:
            for k in ("feat", "npatch", "tlbr"):
                assert torch.equal(out[f"{k}_{tag}"].view(torch.uint8), out[k].view(torch.uint8)), f"{what}: {k} of call '{tag}' differ"
    # the map and the index
    assert out["t2o"].dtype == torch.int32 and out["t2o"].shape == (T, H, W) and out["t2n"].shape == (T, H, W)
    assert torch.equal(out["t2o"], maps["token_to_out"]), f"{what}: token_to_out differs from the reference's"
    assert torch.equal(out["t2n"], maps["token_to_node"]), f"{what}: token_to_node differs from the reference's"
    n = out["tlbr"].shape[0]
    assert torch.equal(torch.bincount(out["t2o"].flatten().long(), minlength=n), out["npatch"].long()), f"{what}: bincount != num_patches"
    tl = out["tlbr"].long()
    assert out["idx"].dtype == torch.int32 and torch.equal(out["idx"].long(), (tl[:, 0] * H + tl[:, 1]) * W + tl[:, 2]), f"{what}: idx"
    if "node_metadata" in out:
        want = maps["node_metadata"]
        assert out["node_metadata"] == want and list(out["node_metadata"]) == list(want), f"{what}: node_metadata differs"
    if not c.pos:
        return
    # pooled rows against the oracle, both modes
    tol = _tol(c.side_dtype)
    for tag, key in (("u", "pos_u"), ("w", "pos_w")):
        if key not in ref:
            continue
        ecoord, ernd = ref[key]
        coord, rnd = out[f"coord_{tag}"], out[f"rnd_{tag}"]
        assert coord.shape == ecoord.shape and coord.dtype == c.side_dtype and rnd.shape == ernd.shape and rnd.dtype == c.side_dtype
        assert bool(torch.isfinite(coord).all()) and bool(torch.isfinite(rnd).all()), f"{what}: pooled rows of a finite side tensor are finite"
        a, b = _worst(rnd, ernd), _worst_rel(coord, ecoord)
        print(f"MEASURED {what} mode={tag} [{c.side_dtype}]: rnd vs oracle {a:.3e}, coord vs oracle (relative) {b:.3e}, bar {tol:.3e}")
        assert a <= tol, f"{what} mode={tag}: pooled cos/sin-like rows {a:.3e} > {tol:.1e}"
        assert b <= tol, f"{what} mode={tag}: pooled coordinate rows {b:.3e} > {tol:.1e} relative"
        assert torch.equal(coord[:, C.ONES].double(), torch.ones(n, dtype=torch.float64)), f"{what} mode={tag}: the ones channel is not exactly 1"
    # weighted mode against the float64 centroid of the map's groups
    bar = 2.0 * C.oracle_deviation(c.side_dtype)
    coord, rnd = out["coord_w"], out["rnd_w"]
    dev = max(C.deviation(coord, ref["centroid"][0]), C.deviation(rnd, ref["centroid"][1]))
    odev = max(C.deviation(ref["pos_w"][0], ref["centroid"][0]), C.deviation(ref["pos_w"][1], ref["centroid"][1]))
    print(f"MEASURED {what} [{c.side_dtype}]: device vs float64 centroid {dev:.3e}, oracle on this case {odev:.3e}, bar {bar:.3e}")
    assert dev <= bar, f"{what}: weighted rows deviate {dev:.3e} from the float64 centroid, bar {bar:.3e} (twice the oracle's own)"
    # sum mode: the accumulated ones ARE the patch count (ones == sum / num_patches == 1 exactly iff sum == num_patches)
    assert torch.equal(coord[:, C.ONES].double() * out["npatch"].double(), out["npatch"].double())


def _expect_refusals(c, xd):
    """What the library cannot serve fails with the reference's error; it never returns rows."""
    import sttm_amd
    from oracle import sttm_oracle as O
    T, _, H, W = c.x.shape
    pe = C.side_tensors(T, H, W, c.Cv, c.side_dtype)
    ped = tuple(p.to(_dev()) for p in pe)
    if c.pos is None:                                         # mixed parity: STTM_ERR_PARITY -> RuntimeError, like the reference
        for mode in (False, True):
            if c.kw["temporal_thresh"] <= 0 and not mode:
                # two reasons to refuse at once: the reference meets the parity first, the library quirk Q11; neither returns rows
                with pytest.raises(RuntimeError, match="parit"):
                    O.get_quadtree_features(c.x, c.thr, pos_embs=pe, pos_emb_weighted_avg=False, **c.kw)
                with pytest.raises((UnboundLocalError, RuntimeError)):
                    sttm_amd.get_quadtree_features(xd, c.thr, pos_embs=ped, pos_emb_weighted_avg=False, **c.kw)
                continue
            with pytest.raises(RuntimeError, match="parit"):
                O.get_quadtree_features(c.x, c.thr, pos_embs=pe, pos_emb_weighted_avg=mode, **c.kw)
            with pytest.raises(RuntimeError, match="parit"):
                sttm_amd.get_quadtree_features(xd, c.thr, pos_embs=ped, pos_emb_weighted_avg=mode, **c.kw)
        kw = dict(c.kw, weighted_avg=True)
        with pytest.raises(RuntimeError):
            O.get_quadtree_features(c.x, c.thr, **kw)
        with pytest.raises(RuntimeError):
            sttm_amd.get_quadtree_features(xd, c.thr, **kw)
    if c.pos == "weighted":                                   # quirk Q11: unweighted pos_embs without the temporal stage
        with pytest.raises(UnboundLocalError):
            O.get_quadtree_features(c.x, c.thr, pos_embs=pe, pos_emb_weighted_avg=False, **c.kw)
        with pytest.raises(UnboundLocalError):
            sttm_amd.get_quadtree_features(xd, c.thr, pos_embs=ped, pos_emb_weighted_avg=False, **c.kw)


def _side(c):
    T, _, H, W = c.x.shape
    return tuple(p.to(_dev()) for p in C.reference(c.name)["pe"]) if c.pos else None


# ----------------------------------------------------------------------------------------------
# 2. consumers x producer paths
# ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(C.SHAPES))
def test_consumers_on_every_producer_path(shape):
    for flag in C.FLAGS:
        name = f"{shape}-{flag}"
        if name not in C.cases():
            continue
        c = C.cases()[name]
        xd, ped = c.x.to(_dev()), _side(c)
        base = _run(c, xd, ped)
        _check_default(c, base, name)
        _expect_refusals(c, xd)
        for opts in C.producer_settings(shape):
            with C.configured(**opts):
                out = _run(c, xd, ped)
            _same_bits(out, base, f"{name} {C.setting_id(opts)}")
        _same_bits(_run(c, xd, ped), base, f"{name} after the settings were restored")


def test_side_tensors_that_differ_from_the_features_in_dtype_and_width():
    """bf16 C=128 features (256-byte rows) with fp32 Cv=32 (128-byte side rows), bf16 Cv=16, fp32 Cv=6 (24-byte rows: no 16-byte
    pack), a strided (not dense) view of a wider table, and a side row wider than the feature row (refused)."""
    import sttm_amd
    for vname in C.SIDE_VARIANTS:
        c = C.cases()[f"A16-{vname}"]
        xd, ped = c.x.to(_dev()), _side(c)
        base = _run(c, xd, ped)
        _check_default(c, base, c.name)
        for opts in (dict(col_walk=2), dict(no_fuse=1), dict(fold_labels=1), dict(gm_split=1)):
            with C.configured(**opts):
                _same_bits(_run(c, xd, ped), base, f"{c.name} {C.setting_id(opts)}")
        # the same values as the leading channels of a table twice as wide: rows are no longer dense (1 x 1 nodes are read through
        # the node rows, not from the tensor)
        wide = tuple(torch.cat([p.permute(0, 2, 3, 1), p.permute(0, 2, 3, 1)], dim=-1).contiguous()[..., :c.Cv].permute(0, 3, 1, 2) for p in ped)
        assert not wide[0].permute(0, 2, 3, 1).is_contiguous()
        for mode, tag in ((False, "u"), (True, "w")):
            r = sttm_amd.get_quadtree_features(xd, c.thr, pos_embs=wide, pos_emb_weighted_avg=mode, **c.kw)
            for got, key in zip(r[3], (f"coord_{tag}", f"rnd_{tag}")):
                assert torch.equal(got.cpu().view(torch.uint8), base[key].view(torch.uint8)), f"{c.name}: strided side tensor, {key}"
    c = C.cases()["A16-plain"]
    sd, cv = C.SIDE_TOO_WIDE
    T, _, H, W = c.x.shape
    pe = tuple(p.to(_dev()) for p in C.side_tensors(T, H, W, cv, D.DTYPES[sd]))
    assert cv * pe[0].element_size() > c.x.shape[1] * c.x.element_size()
    for mode in (False, True):
        with pytest.raises(NotImplementedError, match="wider than the feature rows"):          # STTM_ERR_UNSUPPORTED
            sttm_amd.get_quadtree_features(c.x.to(_dev()), c.thr, pos_embs=pe, pos_emb_weighted_avg=mode, **c.kw)


# ----------------------------------------------------------------------------------------------
# 3. consumers off synth-v1
# ----------------------------------------------------------------------------------------------

def _unmerge_equals_indexing(c, xd, what):
    import sttm_amd
    feat, _, _, t2o, _ = sttm_amd.get_quadtree_features_with_map(xd, c.thr, **c.kw)
    got = sttm_amd.unmerge_tokens(feat, t2o)
    want = feat[t2o.flatten().long()].reshape(*t2o.shape, feat.shape[1])
    assert got.shape == want.shape and got.dtype == feat.dtype
    assert torch.equal(got.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8)), f"{what}: unmerge_tokens differs from indexing"


@pytest.mark.parametrize("fid", C.OD_CLIPS)
def test_consumers_on_off_distribution_clips(fid):
    """Static, duplicated-frame, all-merge, zero-frame, constant and NaN / Inf clips: the longest label chains and largest groups of
    the fixtures.  The side tensors are finite, so the pooled rows are finite and correct also where the features hold NaN / Inf."""
    c = C.cases()[fid]
    od = D.load_od(fid)
    xd, ped = c.x.to(_dev()), _side(c)
    base = _run(c, xd, ped, want_vis=True)
    _check_default(c, base, fid, feats_exp=(od["feat"], od["npatch"], od["tlbr"]))
    _unmerge_equals_indexing(c, xd, fid)
    if fid in C.OD_EVERY_PATH:
        for opts in (dict(no_fuse=1), dict(fold_labels=1), dict(col_walk=2)):
            with C.configured(**opts):
                out = _run(c, xd, ped, want_vis=True)
            _same_bits(out, base, f"{fid} {C.setting_id(opts)}")


def test_consumers_on_a_long_all_merge_clip():
    """T = 128, everything merges into the 16 root cells: groups of up to 2048 patches, representatives 127 frames back, and the
    survivor prefix over 128 frame counts of which all but the first are zero."""
    c = C.cases()["allmerge_T128"]
    ref = C.reference(c.name)
    xd, ped = c.x.to(_dev()), _side(c)
    out = _run(c, xd, ped)
    _check_default(c, out, c.name)
    tl, npatch = out["tlbr"].long(), out["npatch"].long()
    assert tl.shape[0] == 16 and bool((tl[:, 0] == 0).all())
    area = (tl[:, 3] - tl[:, 1]) * (tl[:, 4] - tl[:, 2])
    assert torch.equal(npatch, 128 * area) and int(npatch.max()) == 2048 and int(npatch.sum()) == 128 * 196
    assert torch.equal(torch.bincount(out["t2o"].flatten().long()), npatch)
    # the centroid of a root cell over 128 frames, from its box alone
    centre = torch.stack([torch.full((16,), 63.5, dtype=torch.float64), (tl[:, 1] + tl[:, 3] - 1) / 2.0, (tl[:, 2] + tl[:, 4] - 1) / 2.0], dim=1)
    assert torch.equal(ref["centroid"][0][:, :3], centre)
    dev, bar = C.deviation(out["coord_w"][:, :3], centre), 2.0 * C.oracle_deviation(torch.float32)
    print(f"MEASURED allmerge_T128: (t, y, x) rows vs the root cells' centres {dev:.3e}, bar {bar:.3e}")
    assert dev <= bar
    assert torch.equal(out["coord_w"][:, C.ONES].double() * npatch.double(), npatch.double())
    for opts in (dict(no_fuse=1), dict(gm_split=1)):
        with C.configured(**opts):
            _same_bits(_run(c, xd, ped), out, f"{c.name} {C.setting_id(opts)}")


def test_consumers_on_a_clip_of_one_frame():
    """T = 1: no pairs, every node its own group -- with pos_embs in both modes."""
    c = C.cases()["one_frame"]
    ref = C.reference(c.name)
    assert all(len(v) == 1 for v in ref["maps"]["node_metadata"].values())
    xd, ped = c.x.to(_dev()), _side(c)
    out = _run(c, xd, ped, want_vis=True)
    _check_default(c, out, c.name)
    _unmerge_equals_indexing(c, xd, c.name)
    for opts in (dict(no_fuse=1), dict(col_walk=2), dict(gm_split=64)):
        with C.configured(**opts):
            _same_bits(_run(c, xd, ped, want_vis=True), out, f"{c.name} {C.setting_id(opts)}")
