"""CPU side of the off-distribution tests (tests/_offdist.py): the oracle reproduces the reference on the degenerate clips
(tests/golden/od_*.npz, made by make_golden_offdist.py), and the near-threshold ladders keep the properties the GPU test relies on
-- the oracle equals float64 outside the band, and the band is neither empty nor everything."""
import glob
import os

import pytest
import torch

from oracle import sttm_oracle as O
from tests import _offdist as D
from tests._golden import GOLDEN_DIR


def test_fixture_list_is_the_case_table():
    have = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "od_*.npz")))
    assert have == sorted(D.degenerate_ids())


@pytest.mark.parametrize("fid", D.degenerate_ids())
def test_oracle_reproduces_the_reference_on_degenerate_clips(fid):
    """Indices exact, NaN / Inf positions identical, finite values bit-equal."""
    c = D.load_od(fid)
    thr, kw = D.od_kwargs(c["meta"])
    feat, npatch, tlbr = O.get_quadtree_features(c["x"], thr, **kw)
    assert tlbr.dtype == torch.int32 and npatch.dtype == torch.int32
    assert torch.equal(tlbr, c["tlbr"]) and torch.equal(npatch, c["npatch"])
    assert D.bits_equal_nan_aware(feat, c["feat"])
    assert os.path.getsize(os.path.join(GOLDEN_DIR, fid + ".npz")) < 512 * 1024


@pytest.mark.parametrize("kind", D.OCTREE_KINDS)
def test_octree_oracle_reproduces_the_reference_on_degenerate_clips(kind):
    """The octree oracle is the referee nowhere here, but it has to be right off-distribution too: same tokens, same NaN / Inf
    pattern, finite values within test_octree_oracle_golden.py's 1e-6."""
    from oracle import octree_oracle as OC
    x, feat = D.load_odoct(kind)
    assert torch.equal(x.contiguous().view(torch.int32), D.build_octree_degenerate(kind).contiguous().view(torch.int32))
    D.check_features_nan_aware(OC.get_octree_features(x, D.OCTREE_THR, D.OCTREE_ROOT), feat, kind, tol=1e-6)


def test_degenerate_clips_do_what_their_names_say():
    """The fixtures hold the cases they are meant to hold (a changed builder would otherwise pin something else silently)."""
    n = {fid: D.load_od(fid) for fid in ("od_zero_video_f32", "od_const_f32", "od_static_f32", "od_dup_frames_f32", "od_inf_block_f32",
                                         "od_nan_elem_f32", "od_scale_p62_f32", "od_scale_m70_f32", "od_allmerge_f32", "od_overflow_t48_w_f16")}
    assert n["od_zero_video_f32"]["tlbr"].shape[0] == 1176 and n["od_scale_p62_f32"]["tlbr"].shape[0] == 1176
    assert n["od_scale_m70_f32"]["tlbr"].shape[0] == 1176
    assert n["od_const_f32"]["tlbr"].shape[0] == 16 and n["od_static_f32"]["tlbr"].shape[0] == 118
    assert n["od_dup_frames_f32"]["tlbr"].shape[0] == 485
    tl = n["od_inf_block_f32"]["tlbr"]
    blk = tl[(tl[:, 0] == 1) & (tl[:, 1] >= 4) & (tl[:, 3] <= 6) & (tl[:, 2] >= 8) & (tl[:, 4] <= 10)]
    assert blk.shape[0] == 4, "the reference splits the block with an Inf channel into its four leaves"
    assert int(torch.isnan(n["od_nan_elem_f32"]["feat"]).sum()) == 1
    am = n["od_allmerge_f32"]
    assert am["tlbr"].shape[0] == 16 and int(am["npatch"].sum()) == 32 * 196 and int(am["npatch"].max()) == 512
    assert int(torch.isinf(n["od_overflow_t48_w_f16"]["feat"].float()).sum()) > 0, "the float16 group sums should overflow"


@pytest.mark.parametrize("spec", D.ALL_LADDERS, ids=D.ladder_id)
def test_ladder_band(spec):
    """1a on the CPU: outside the band the oracle decides as float64 does.  1b: the band holds enough decisions to measure a flip
    rate and few enough for the hard assertion to mean something (shares stated by the issue from the reference's own error)."""
    lad = D.ladder(*spec)
    got = lad.oracle_decisions(slow_ver=True) if spec in D.SLOW_LADDERS else lad.oracle_decisions()
    assert torch.equal(got, lad.want32), "the decoded oracle decisions are not `sim_fp32 >= threshold`"
    if lad.kind == "spatial" and lad.run_tthr > 0:
        # the temporal stage is on (that is what reaches the column walk) but keeps no pair: same nodes as the spatial stage alone
        both = O.get_quadtree_features(lad.x, lad.thr, **lad.kwargs())
        alone = O.get_quadtree_features(lad.x, lad.thr, **lad.kwargs(temporal_thresh=-1.0))
        assert torch.equal(both[2], alone[2]) and torch.equal(both[1], alone[1]), "a spatial ladder video merged temporally"
    lad.assert_outside_band(got, "oracle")
    n, out = lad.outside.numel(), int(lad.outside.sum())
    if lad.kind == "spatial":
        assert lad.far > lad.level + 0.03, "the three other slots must stay far above the threshold"
    if lad.dtype == torch.float32:
        assert out >= 0.60 * n, f"only {out} of {n} decisions outside the band (eps {lad.eps:.2e})"
        assert n - out >= 100, f"only {n - out} of {n} decisions inside the band (eps {lad.eps:.2e})"
    else:
        assert out >= 0.85 * n, f"only {out} of {n} decisions outside the band (eps {lad.eps:.2e})"
    assert bool(lad.want64.any()) and bool((~lad.want64).any())


@pytest.mark.parametrize("setting", D.HEAVY_SETTINGS)
def test_heavy_family_meets_the_index_exact_share_on_the_reference_side(setting):
    """The north star asks for >= 90 % of the videos index-exact.  A video is held to that when all its decisions lie outside the
    band; at most 10 % of a setting's 16 videos may fall outside that class (a property of the seeds, checked here without a device).
    The crowded setting must also stay crowded: the reference keeps between 20 % and 80 % of the tokens at 0.94/0.82."""
    cases = [(c, D.heavy_case(setting, *c, seed)) for c in D.HEAVY_COMBOS for seed in D.HEAVY_SEEDS]
    in_band = [m for _, (_, m) in cases if not m.decisive]
    print(f"{setting}: {len(in_band)} of {len(cases)} videos have a decision inside the band; eps spatial "
          f"{max(m.eps_sp for _, (_, m) in cases):.2e}, temporal {max(m.eps_tp for _, (_, m) in cases):.2e}")
    assert len(in_band) <= 0.10 * len(cases)
    for (C, d, thr, tthr), (x, m) in cases:
        kept = m.out[2].shape[0] / (16 * 196)
        if setting == "massive" and thr == 0.85:
            assert m.out[2].shape[0] == 16, "the massive channels should merge everything into the 16 root cells"
        if setting == "crowded" and thr == 0.94:
            assert 0.20 <= kept <= 0.80, f"C={C} {d}: the reference keeps {kept:.2f} of the tokens"


def test_margins_recorder_leaves_the_oracle_unchanged():
    from sttm_amd.synth import synth_video
    x = synth_video(6, 64, 14, 14, seed=3)
    m = D.Margins(x, 0.85, 0.55, 1)
    exp = O.get_quadtree_features(x, 0.85, 0.55, 1)
    assert all(torch.equal(a, b) for a, b in zip(m.out, exp))
    assert m.n_decisions > 16 * 6 and m.eps_sp < 1e-5 and m.eps_tp < 1e-5
