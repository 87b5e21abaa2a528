"""CPU side of the octree off-distribution tests (tests/_octree_offdist.py): the fixtures are what their builders make and the
oracle reproduces the reference on them; the ladders keep the properties the GPU test relies on; every video of the dispatch table
has no decision inside the band and emits nodes from at least two pyramid levels."""
import glob
import os

import pytest
import torch

from oracle import octree_oracle as OC
from tests import _octree_offdist as X
from tests import _offdist as D
from tests._golden import GOLDEN_DIR, OCTREE_GOLDEN


def test_fixture_list_is_the_case_table():
    have = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "odo_*.npz")))
    assert have == sorted(X.deg_file(k, s) for s in X.DEG_SIDES for k in X.DEG_KINDS)
    assert not any("odo_" in p for p in OCTREE_GOLDEN)
    largest = max(os.path.getsize(p) for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")) if "odo_" not in p)
    assert all(os.path.getsize(os.path.join(GOLDEN_DIR, n + ".npz")) < min(largest, 512 * 1024) for n in have)


@pytest.mark.parametrize("case", X.deg_cases(), ids=X.deg_id)
def test_oracle_reproduces_the_reference_on_odd_side_degenerate_clips(case):
    """Bit-checked against the builder; same rows as the reference, NaN / Inf at the same places, finite values bit-equal -- at every
    threshold, the constant video at 1.0 included (the oracle runs the reference's own fp32 operators)."""
    kind, side, thr = case
    x, feat = X.load_deg(case)
    assert torch.equal(x.contiguous().view(torch.int32), X.build_deg(kind, side).contiguous().view(torch.int32))
    assert x.shape[0] == 2 * side + 1 and x.shape[1] <= 16
    out = OC.get_octree_features(x, thr, 0)
    assert out.shape == feat.shape and D.bits_equal_nan_aware(out, feat)


def test_degenerate_clips_do_what_their_names_say():
    rows = {X.deg_id(c): X.load_deg(c)[1].shape[0] for c in X.deg_cases()}
    for side in X.DEG_SIDES:
        T, roots, leaves = 2 * side + 1, X.root_count(2 * side + 1, side), (2 * side + 1) * side * side
        f = lambda kind, thr: rows[X.deg_id((kind, side, thr))]                    # noqa: E731
        assert f("const", 0.8) == f("static", 0.8) == f("const", -0.3) == f("zero_video", 0.0) == f("scale_m70", 0.0) == roots == 20
        assert f("zero_video", 0.8) == f("scale_m70", 0.8) == f("const", 1.5) == f("zero_origin", 1.5) == leaves
        # a zero / NaN / Inf origin leaf fails every alias comparison of its cube: cells with missing slots split where the plain
        # clip's stop, and not even a threshold below every cosine merges that cube into its roots
        plain = f("nan_inner", 0.8)
        assert f("zero_origin", 0.8) > plain and f("nan_origin", 0.8) > plain and f("inf_origin", 0.8) > plain
        assert f("nan_origin", -0.3) > roots and f("inf_origin", -0.3) > roots and f("zero_origin", -0.3) == roots
        assert roots <= f("const", 1.0) < leaves, "the reference's fp32 rounding decides the constant video at 1.0"
        e = X.deg_expect(("nan_origin", side, 0.8))
        assert e.pinned and len(e.m.levels_emitting) >= 2
    # the scalings reach what they are meant to reach: fp32 norm overflow, and squared norms below the 1e-16 clamp
    x = X.build_deg("scale_p62", 7).permute(0, 2, 3, 1)
    assert bool(torch.isinf((x * x).sum(-1)).any())
    x = X.build_deg("scale_m70", 7).permute(0, 2, 3, 1)
    assert float((x * x).sum(-1).max()) < 1e-16


@pytest.mark.parametrize("case", X.deg_cases(), ids=X.deg_id)
def test_degenerate_clip_margins(case):
    """Which clips pin the reference's rows: all but the threshold-1.0 runs of the constant and static clips.  The zero / NaN / Inf
    origin clips have in-band slots at 1.0 too, but only in cells another slot fails: their result is determined.  What the GPU test
    asks of the device holds for the reference's own rows."""
    kind, side, thr = case
    e = X.deg_expect(case)
    print(f"{X.deg_id(case)}: eps {e.m.eps:.2e}, {e.in_band} of {e.m.n_decisions} decisions in the band (zero similarities aside), "
          f"{e.n_open} open cells, reference rows {e.feat.shape[0]}")
    assert e.pinned == (thr != 1.0 or kind not in ("const", "static"))
    if e.pinned:
        return
    rem = OC.O.get_quadtree_features(e.x[e.T - 1:], thr, -1.0, 0)[0].shape[0]
    cube = e.feat[:e.feat.shape[0] - rem]
    assert e.enumerable == (kind == "static") and e.n_min < e.n_max
    if e.enumerable:
        k = e.check_open(cube, X.deg_id(case) + " (reference)")
        print(f"{X.deg_id(case)}: reference cube rows {cube.shape[0]} in [{e.n_min}, {e.n_max}], {k} of {e.n_open} open cells stopped")
        with pytest.raises(AssertionError):                      # the check bites: two rows swapped, or one row dropped
            e.check_open(torch.cat([cube[1:2], cube[0:1], cube[2:]]), "swapped")
        with pytest.raises(AssertionError):
            e.check_open(cube[:-1], "dropped")
    else:
        n = e.check_free(cube, X.deg_id(case) + " (reference)")
        print(f"{X.deg_id(case)}: reference cube rows {n} in [{e.n_min}, {e.n_max}]")
        assert e.rows_are_cells_bitwise(cube), "the reference's rows are the oracle's pooled means of the constant token"
        assert e.n_min == 2 * 8, "every in-band slot passing merges the constant cubes into their roots"


@pytest.mark.parametrize("spec", X.LADDERS, ids=X.ladder_id)
def test_ladder_band(spec):
    lad = X.oct_ladder(*spec)
    exp = OC.get_octree_features(lad.x, lad.thr, 0)
    assert torch.equal(exp, lad.m.out32), "the restated traversal differs from the oracle's"
    got = lad.decode(exp)
    assert torch.equal(got, lad.want32), "the decoded oracle decisions are not `sim_fp32 >= threshold`"
    assert torch.equal(lad.decode(lad.m.out64), lad.want64), "the float64-decided traversal does not decode to the float64 decisions"
    lad.assert_outside_band(got, "oracle")
    by_rung = lad.in_band_by_rung()
    n, out = lad.outside.numel(), int(lad.outside.sum())
    print(f"{X.ladder_id(spec)}: eps {lad.eps:.2e}, in the band by rung {by_rung}, {n} decisions, whole-video eps {lad.m.eps:.2e}")
    assert lad.far > lad.level32 + 0.03, "the seven other slots must stay far above the threshold"
    assert bool(lad.want64.any()) and bool((~lad.want64).any())
    # every decision off the ladder level is far from the threshold: leaf blocks of an upper ladder have cosine 1, every level above
    # a ladder compares unrelated means
    for l, s64 in enumerate(lad.m.sim64):
        if l != lad.lad_level:
            assert float((s64 - lad.level32).abs().min()) > 0.03
    if lad.dtype == torch.float32:
        assert by_rung[1e-5] == 0 and by_rung[1e-4] == 0 and by_rung[1e-7] + by_rung[1e-6] > 0
    else:
        assert out >= 0.85 * n          # 16-bit inputs move a block's similarity off its rung; the band itself is as narrow


CHECKED = X.ORDINARY + X.SCAN_CASES


@pytest.mark.parametrize("spec", sorted(set(CHECKED), key=CHECKED.index), ids=X.case_id)
def test_dispatch_cases_have_no_decision_in_the_band(spec):
    c = X.case(*spec)
    m = c.m
    print(f"{X.case_id(spec)}: eps {m.eps:.2e}, {m.in_band} of {m.n_decisions} decisions in the band, remainder {c.rem_in_band}, levels "
          f"emitting {m.levels_emitting}, {c.exp.shape[0]} rows")
    assert m.in_band == 0 and c.rem_in_band == 0, "change the seed of this case: a decision lies inside the band"
    n_cube = m.out32.shape[0]
    assert torch.equal(c.exp[:n_cube], m.out32) and torch.equal(m.out32, m.out64)
    if len(m.levels) >= 2 and abs(spec[5]) < 1.5:        # (a one-level pyramid, or a threshold beyond every cosine, has one level)
        assert len(m.levels_emitting) >= 2, "this case does not emit nodes from two pyramid levels"


def test_grid_stride_case():
    """766 cubes of side 14 at root_level 1: more side-7 cells than the waves of one full k_oct_stop launch, and the cells of the
    second pass of that loop decide differently from an all-split or all-stop default: the last cube holds a stopped inner cell."""
    c = X.case(*X.GRID_CASE)
    assert c.m.levels[1].shape[:4] == (766, 7, 7, 7) and 766 * 343 > 65536 * 4
    assert c.m.in_band == 0 and c.rem_in_band == 0 and c.m.drop == 3
    assert len(c.m.levels_emitting) == 3 and c.m.last_cube_has_stopped_inner_cell()
    assert torch.equal(c.exp[:c.m.out32.shape[0]], c.m.out32)
    late = c.m.stop32[1].reshape(-1)[65536 * 4:]
    assert bool(late.any()) and bool((~late).any())


def test_side_table_covers_every_root_level():
    for side in X.SIDES:
        n = len(OC.side_levels(side))
        assert sorted(s[6] for s in X.SIDE_CASES if s[3] == side) == list(range(-n, n))
        with pytest.raises(IndexError):
            OC.get_octree_features(X.case(*[s for s in X.SIDE_CASES if s[3] == side][0]).x, 0.8, n)
        with pytest.raises(IndexError):
            OC.get_octree_features(X.case(*[s for s in X.SIDE_CASES if s[3] == side][0]).x, 0.8, -n - 1)
    assert len(OC.side_levels(33)) == 6
