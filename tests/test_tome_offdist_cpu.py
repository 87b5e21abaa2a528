"""CPU side of the ToMe off-distribution tests (tests/_tome_offdist.py): the oracle reproduces the reference on every family
(tests/golden/tomeod_*.npz, made by make_golden_tome_offdist.py), the fixtures hold the cases their names promise, and every committed
clip is one the reference alone is well determined on."""
import glob
import os

import pytest
import torch

from oracle import sttm_oracle as O
from tests import _tome_offdist as D
from tests._golden import GOLDEN_DIR
from tests._offdist import DTYPES


def test_fixture_list_is_the_family_table():
    have = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "tomeod_*.npz")))
    assert have == sorted(D.fixture_ids())


@pytest.mark.parametrize("fid", D.fixture_ids())
def test_oracle_reproduces_the_reference(fid):
    """Ids exact, NaN / Inf positions identical, finite values bit-equal -- for every ratio of the family; the committed input is
    what the family's builder makes."""
    c = D.load_fixture(fid)
    m = c["meta"]
    assert os.path.getsize(os.path.join(GOLDEN_DIR, fid + ".npz")) < 128 * 1024
    rebuilt = D.build(m["case"], m["dtype"], m["seed"])
    assert D.bits_equal_nan_aware(rebuilt.permute(0, 2, 3, 1), c["x"].permute(0, 2, 3, 1)), "the builder no longer makes the committed input"
    assert m["seed"] == D.seed_of(m["case"], m["dtype"]) and tuple(m["ratios"]) == tuple(D.FAMILIES[m["case"]][4])
    for ratio, (efeat, eidx) in c["out"].items():
        feat, idx = O.get_tome_features(c["x"], ratio, "video", m["n_head"])
        assert idx.dtype == torch.int64 and torch.equal(idx, eidx), f"{fid} r={ratio}: ids differ"
        assert D.bits_equal_nan_aware(feat, efeat), f"{fid} r={ratio}: features differ"
        assert feat.shape[0] == D.kept_count(m["T"] * m["H"] * m["W"], ratio)


@pytest.mark.parametrize("fid", D.fixture_ids())
def test_committed_clips_are_well_determined(fid):
    """The same loop with float64 scores takes the same node_idx and keeps the same ids, and no cut separates tied row maxima."""
    c = D.load_fixture(fid)
    for ratio in c["out"]:
        ok, why = D.well_determined(c["x"], ratio, c["meta"]["n_head"])
        assert ok, f"{fid} r={ratio}: {why}"


@pytest.mark.parametrize("fid", D.fixture_ids())
def test_device_rules_reproduce_the_reference(fid):
    """What the GPU test asks of the kernels is satisfiable: the loop with the kernels' own rules where the reference leaves a choice
    (stable ranking, sources in rank order, 16-bit sums rounded once) meets every fixture under the GPU test's comparison."""
    c = D.load_fixture(fid)
    for ratio, (efeat, eidx) in c["out"].items():
        feat, idx = D.tome_with_device_rules(c["x"], ratio, c["meta"]["n_head"])
        D.assert_matches_fixture(feat, idx, efeat, eidx, ratio, f"{fid} r={ratio}")


def test_reference_argsort_is_not_stable_on_ties():
    """Why the families avoid a cut through tied keys: ATen's CPU `argsort(descending=True)` returns tied keys (all NaN, or all equal)
    in index order only up to 16 of them.  (If a later torch makes it stable this test says so and the restriction can go.)"""
    for v in (torch.full((74,), float("nan")), torch.ones(74)):
        assert torch.equal(v[:16].argsort(descending=True), torch.arange(16))
        assert not torch.equal(v.argsort(descending=True), torch.arange(74))
        assert torch.equal(v.argsort(descending=True, stable=True), torch.arange(74))


def _trace(fid, ratio):
    c = D.load_fixture(fid)
    return c, D.tome_trace(c["x"], ratio, c["meta"]["n_head"])[2]


def test_families_do_what_their_names_say():
    """A changed builder would otherwise pin something else silently."""
    # a poisoned b-token: node_max NaN for every a-row, node_idx the (first) poisoned b-row
    for fid, j in (("tomeod_zero_b_token_f32", 20), ("tomeod_nan_elem_b_bf16", 20), ("tomeod_inf_elem_b_f32", 20), ("tomeod_nan_two_b_f32", 20),
                   ("tomeod_nan_b_first_f32", 0), ("tomeod_tiny_b_token_f32", 20), ("tomeod_tiny_b_token_bf16", 20), ("tomeod_nan_b_last_bf16", 97), ("tomeod_nan_head4_f32", 20), ("tomeod_nan_elem_b_14_f32", 150)):
        _, rec = _trace(fid, 0.5)
        best, arg, _ = rec[0]
        assert bool(torch.isnan(best.float()).all()) and bool((arg == j).all()), fid
    # a poisoned a-token: its own row is (NaN, 0), every other row finite
    for fid in ("tomeod_zero_a_token_f32", "tomeod_nan_elem_a_bf16", "tomeod_inf_elem_a_f32", "tomeod_zero_a_token_cut_bf16",
                "tomeod_tiny_a_token_f32", "tomeod_tiny_a_token_bf16"):
        _, rec = _trace(fid, 0.5)
        best, arg, _ = rec[0]
        nan = torch.isnan(best.float())
        assert nan.nonzero().flatten().tolist() == [20] and int(arg[20]) == 0, fid
    # the tiny token's unit row is +-Inf without a NaN in it
    for d in ("f32", "bf16"):
        c = D.load_fixture(f"tomeod_tiny_b_token_{d}")
        t = c["x"].permute(0, 2, 3, 1).reshape(-1, 32)[41:42]
        u = (t / t.norm(dim=-1, keepdim=True)).float()
        assert bool(torch.isinf(u).all()) and bool((t != 0).all())
    # a zero frame: the zero a-rows are (NaN, 0), the clean ones (NaN, first zero b-row)
    c, rec = _trace("tomeod_zero_frame_f32", 0.5)
    best, arg, _ = rec[0]
    zero_a = (c["x"].permute(0, 2, 3, 1).reshape(-1, 32)[0::2] == 0).all(dim=1)
    assert bool(torch.isnan(best).all()) and bool((arg[zero_a] == 0).all()) and bool((arg[~zero_a] == 24).all()) and int(zero_a.sum()) == 24
    # norms: 1e-30 underflows (unit rows +-inf, every score NaN), 1e+20 overflows (unit rows 0, every score 0, first j wins)
    for d in ("f32", "bf16"):
        _, rec = _trace(f"tomeod_scale_1e-30_{d}", 0.5)
        assert bool(torch.isnan(rec[0][0].float()).all()) and bool((rec[0][1] == 0).all())
        _, rec = _trace(f"tomeod_scale_1e+20_{d}", 0.5)
        assert bool((rec[0][0].float() == 0).all()) and bool((rec[0][1] == 0).all())
    # exact ties: a constant clip sends everything to b-row 0; on duplicated 7 x 7 frames every a-token's copy is a b-token
    _, rec = _trace("tomeod_const_video_f32", 0.5)
    assert bool((rec[0][1] == 0).all()) and float(rec[0][0].min()) > 0.999
    c, rec = _trace("tomeod_dup_frames_f32", 0.5)
    tok = c["x"].permute(0, 2, 3, 1).reshape(-1, 32)
    assert bool((tok[0::2] == tok[1::2][rec[0][1]]).all()), "every a-token should be matched with its exact copy"
    # float16: input elements at Inf; merge sums past 65 504
    c = D.load_fixture("tomeod_f16_scale_inf_f16")
    assert int(torch.isinf(c["x"].float()).sum()) > 0
    c = D.load_fixture("tomeod_f16_merge_overflow_f16")
    assert int(torch.isinf(c["x"].float()).sum()) == 0 and 100 < float(c["x"].float().abs().max()) < 1000
    assert all(int(torch.isinf(f.float()).sum()) > 0 for f, _ in c["out"].values()), "the float16 merge sums should overflow"
    assert max(c["out"]) >= 0.85
    # every family has 0.5 and a ratio of at least two iterations
    for name, (_, (T, _C, H, W), _, dts, ratios) in D.FAMILIES.items():
        n = T * H * W
        assert 0.5 in ratios and any(D.kept_count(n, r) < n - n // 2 for r in ratios), name
        assert all(d in DTYPES for d in dts)


def test_dense_match_reference_has_torch_max_semantics():
    x = torch.randn(40, 16)
    x[7, 3] = float("nan")                     # b-row 3
    x[10] = 0                                  # a-row 5
    best, arg = D.dense_match_reference(x, torch.float32)
    assert bool(torch.isnan(best).all()) and int(arg[5]) == 0 and bool((arg[torch.arange(20) != 5] == 3).all())
