"""GPU parity of the quadtree (STTM) path away from synth-v1 (tests/_offdist.py):

1. near-threshold ladders through every path with its own decision arithmetic or reduction order -- outside the band
   eps = 2 * max |sim_oracle_fp32 - sim_float64| (computed on the CPU, from the reference side alone) every device decision must equal
   the float64 decision;
2. degenerate clips (zero tokens / frames / videos, duplicated and static frames, a constant video, NaN / Inf elements, scalings to
   the eps clamp and past fp32 norm overflow, clips in which everything merges) against the reference's own outputs
   (tests/golden/od_*.npz): same node set, same NaN / Inf pattern, finite features within the bars;
3. the heavy-tailed, massive-activation family of sttm_amd.synth.heavy_video against the oracle;
4. the octree baseline, which decides with the same division-free test, on Inf / overflow / zero / NaN clips against the
   reference's outputs (tests/golden/odoct_*.npz).
"""
import pytest
import torch

from tests import _offdist as D

pytestmark = pytest.mark.gpu

LABEL_DEFAULTS = dict(fold_labels=0, no_fuse=0, force_gmem_labels=0, fold_kb=64, pairs_seg=0, pairs_nt=0, pairs_var=0, no_dense=0, k1_var=0)
COL_DEFAULTS = dict(col_walk=0, col_frames=8, col_cap=0, col_pb=0)


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


class _configured:
    """sttm_configure switches for the duration of a block; none of them may change a result."""

    def __init__(self, **opts):
        self.opts = opts

    def __enter__(self):
        from sttm_amd import _lib
        _lib.configure(**self.opts)

    def __exit__(self, *exc):
        from sttm_amd import _lib
        torch.cuda.synchronize()
        _lib.configure(k1_split=0, **LABEL_DEFAULTS, **COL_DEFAULTS)


# ----------------------------------------------------------------------------------------------
# 1. near-threshold ladders
# ----------------------------------------------------------------------------------------------

def _device_decisions(lad, **extra):
    from sttm_amd import get_quadtree_features
    out = get_quadtree_features(lad.x.to(_dev()), lad.thr, **lad.kwargs(**extra))
    return lad.decode(out[2])


def _report(lad, got, what):
    """The figures of 1d, printed before the assertion (pytest -s / the ladder tool show them)."""
    ins = int((~lad.outside).sum())
    print(f"{what}: eps {lad.eps:.2e}, {ins} of {lad.outside.numel()} decisions in the band, in-band flips device/oracle "
          f"{int(((got != lad.want32) & ~lad.outside).sum())}, device/float64 {int(((got != lad.want64) & ~lad.outside).sum())}, "
          f"oracle/float64 {int(((lad.want32 != lad.want64) & ~lad.outside).sum())}")


def lad_runs_temporal(spec):
    return D.ladder(*spec).run_tthr > 0


def _assert_ladder(lad, got, what):
    _report(lad, got, what)
    lad.assert_outside_band(got, what)


@pytest.mark.parametrize("spec", D.DEFAULT_LADDERS, ids=D.ladder_id)
def test_ladder_default_path(spec):
    lad = D.ladder(*spec)
    _assert_ladder(lad, _device_decisions(lad), D.ladder_id(spec))


@pytest.mark.parametrize("spec", D.COLWALK_LADDERS, ids=D.ladder_id)
@pytest.mark.parametrize("opts", [dict(col_walk=2), dict(col_walk=2, col_frames=3), dict(pairs_var=9)],
                         ids=lambda o: "+".join(f"{k}={v}" for k, v in o.items()))
def test_ladder_column_walk_and_general_pair_kernel(spec, opts):
    """The spatial and pair tests inside the column walk (col_walk=2 forces it for a one-video call) and the general pair kernel.
    Both exist only while the temporal stage is on: the spatial ladder runs with the preset's temporal threshold, which keeps no pair
    of its unrelated blocks (tests/_offdist.py, Ladder.run_tthr)."""
    assert lad_runs_temporal(spec)
    lad = D.ladder(*spec)
    with _configured(**opts):
        got = _device_decisions(lad)
    _assert_ladder(lad, got, f"{D.ladder_id(spec)} {opts}")


@pytest.mark.parametrize("spec", D.HEAD_LADDERS, ids=D.ladder_id)
def test_ladder_per_head(spec):
    """head_dim set: the spatial per-head mean and the pair path that divides by (sqrtf(na) + 1e-8f) * (sqrtf(nb) + 1e-8f)."""
    lad = D.ladder(*spec)
    _assert_ladder(lad, _device_decisions(lad), D.ladder_id(spec))


@pytest.mark.parametrize("spec", D.SLOW_LADDERS, ids=D.ladder_id)
def test_ladder_slow_ver(spec):
    lad = D.ladder(*spec)
    _assert_ladder(lad, _device_decisions(lad, slow_ver=True), D.ladder_id(spec) + " slow_ver")


@pytest.mark.parametrize("spec", D.NODES_LADDERS, ids=D.ladder_id)
def test_ladder_standalone_temporal_entry_point(spec):
    """temporal_merge_nodes on the list of all leaves: the norms come from the node-ingest kernel, not from the spatial stage."""
    from sttm_amd.quadtree_interface import temporal_merge_nodes
    lad = D.ladder(*spec)
    T, H, W, C = lad.T, lad.H, lad.W, lad.C
    feats = lad.x.permute(0, 2, 3, 1).reshape(T * H * W, C)
    t, y, x = torch.meshgrid(torch.arange(T), torch.arange(H), torch.arange(W), indexing="ij")
    tlbr = torch.stack([t, y, x, y + 1, x + 1], dim=-1).reshape(-1, 5).to(torch.int32)
    out = temporal_merge_nodes(feats.to(_dev()), tlbr.to(_dev()), lad.tthr, grid=(T, H, W), root_level=1)
    _assert_ladder(lad, lad.decode(out[2]), D.ladder_id(spec) + " temporal_merge_nodes")


@pytest.mark.parametrize("specs", [D.BATCH_LADDERS, D.BATCH_SPATIAL_LADDERS], ids=["temporal", "spatial"])
@pytest.mark.parametrize("col_walk", [0, 1])
def test_ladder_batch_entry_point(specs, col_walk):
    """Four ladder videos of two lengths in one get_quadtree_features_batch call; with col_walk=1 the launch sets of several videos
    run the column walk."""
    from sttm_amd.quadtree_interface import get_quadtree_features_batch
    lads = [D.ladder(*s) for s in specs]
    assert all(l.run_tthr > 0 for l in lads)              # the column walk needs the temporal stage
    with _configured(col_walk=col_walk):
        outs = get_quadtree_features_batch([l.x.to(_dev()) for l in lads], lads[0].thr, **lads[0].kwargs())
    assert len(outs) == len(lads)
    for spec, lad, out in zip(specs, lads, outs):
        _assert_ladder(lad, lad.decode(out[2]), f"batch col_walk={col_walk} {D.ladder_id(spec)} T={lad.T}")


@pytest.mark.parametrize("spec", D.WIDE_LADDERS, ids=D.ladder_id)
def test_ladder_channel_tiled_wide_rows(spec):
    """fp32 C = 8192 runs the channel-tiled spatial stage: partial statistics per tile."""
    lad = D.ladder(*spec)
    _assert_ladder(lad, _device_decisions(lad), D.ladder_id(spec))


@pytest.mark.parametrize("spec", D.DEEP_LADDERS, ids=D.ladder_id)
@pytest.mark.parametrize("k1_split", [0, -1])
def test_ladder_deep_tree(spec, k1_split):
    """A 6-level tree (64 x 64, root_level 0): the split form (one workgroup per 3-level block + a pass over the upper levels) and
    the one-workgroup form.  The ladder sits at the leaf level; every level above splits by construction."""
    lad = D.ladder(*spec)
    with _configured(k1_split=k1_split):
        got = _device_decisions(lad)
    _assert_ladder(lad, got, f"{D.ladder_id(spec)} k1_split={k1_split}")


# ----------------------------------------------------------------------------------------------
# 2. degenerate clips
# ----------------------------------------------------------------------------------------------

def _run_od(c, **extra):
    from sttm_amd import get_quadtree_features
    thr, kw = D.od_kwargs(c["meta"])
    kw.update(extra)
    return get_quadtree_features(c["x"].to(_dev()), thr, **kw)


@pytest.mark.parametrize("fid", D.degenerate_ids())
def test_degenerate_clip_equals_the_reference(fid):
    c = D.load_od(fid)
    out = _run_od(c)
    m = c["meta"]
    if m["kw"]["threshold"] >= 1.0:
        # whether a vector's fp32 self-cosine rounds to 1.0 depends on the summation order; structure only
        assert int(out[1].sum()) == m["T"] * m["H"] * m["W"] and out[0].shape[0] == out[2].shape[0] == out[1].shape[0]
        return
    D.check_nan_aware(out, (c["feat"], c["npatch"], c["tlbr"]), fid)


@pytest.mark.parametrize("name", ["zero_tokens", "zero_video", "nan_elem", "inf_elem", "inf_block", "scale_p62", "scale_m70", "static"])
@pytest.mark.parametrize("dname", ["float32", "bfloat16", "float16"])
def test_degenerate_clip_per_head_against_oracle(name, dname):
    """The per-head similarity (head_dim = 16: two heads) has its own arithmetic in both stages; the referee is the oracle."""
    from oracle import sttm_oracle as O
    from sttm_amd import get_quadtree_features
    x = D.build_degenerate(name, D.DTYPES[dname])
    exp = O.get_quadtree_features(x, 0.85, 0.55, 1, head_dim=16)
    D.check_nan_aware(get_quadtree_features(x.to(_dev()), 0.85, 0.55, 1, head_dim=16), exp, f"{name} {dname} head_dim=16")


F16_CLIPS = ["zero_tokens", "zero_frame", "zero_block", "zero_video", "dup_frames", "static", "const", "nan_elem", "inf_elem", "inf_block", "pm_inf",
             "scale_p40", "scale_m40"]


@pytest.mark.parametrize("name", F16_CLIPS)
def test_degenerate_clip_float16_against_oracle(name):
    """The base-clip cases in float16 (fixtures exist for float32 and bfloat16): the referee is the oracle.  2^40 takes every element
    to +-Inf in float16 and 2^-40 to zero."""
    from oracle import sttm_oracle as O
    from sttm_amd import get_quadtree_features
    x = D.build_degenerate(name, torch.float16)
    exp = O.get_quadtree_features(x, 0.85, 0.55, 1)
    D.check_nan_aware(get_quadtree_features(x.to(_dev()), 0.85, 0.55, 1), exp, f"{name} float16")


LONG_CHAIN_CLIPS = ["od_static_f32", "od_dup_frames_f32", "od_allmerge_f32", "od_allmerge_w_f32", "od_allmerge_bf16", "od_static_bf16"]


def _label_paths():
    from tests.test_hip_parity import LABEL_PATHS
    return LABEL_PATHS + [dict(col_walk=2), dict(col_walk=2, col_frames=3, col_cap=2)]


@pytest.mark.parametrize("opts", _label_paths(), ids=lambda o: "+".join(f"{k}={v}" for k, v in o.items()) or "default")
def test_long_label_chains_on_every_label_path(opts):
    """Static, duplicated-frame and all-merge clips hold the longest label chains and the largest groups of the suite (32 frames x
    every cell of a root): every way the label stage can run gives the reference's result, bit-identical to the default path."""
    for fid in LONG_CHAIN_CLIPS:
        c = D.load_od(fid)
        base = _run_od(c)
        with _configured(**opts):
            out = _run_od(c)
        D.check_nan_aware(out, (c["feat"], c["npatch"], c["tlbr"]), f"{fid} {opts}")
        for u, v, name in zip(out, base, ("features", "num_patches", "tlbr")):
            assert torch.equal(u, v), f"{fid} {opts}: {name} differ from the default path"


@pytest.mark.parametrize("col_walk", [0, 1])
def test_long_label_chains_through_the_batch_entry_point(col_walk):
    """One call over clips of two shapes, bit-identical to one call per video; col_walk=1 runs the launch sets on the column walk."""
    from sttm_amd.quadtree_interface import get_quadtree_features_batch
    cs = [D.load_od(f) for f in ("od_static_f32", "od_allmerge_f32", "od_dup_frames_f32", "od_const_f32", "od_allmerge_f32", "od_zero_frame_f32")]
    single = [_run_od(c) for c in cs]
    thr, kw = D.od_kwargs(cs[0]["meta"])
    with _configured(col_walk=col_walk):
        batch = get_quadtree_features_batch([c["x"].to(_dev()) for c in cs], thr, **kw)
    for c, a, b in zip(cs, batch, single):
        D.check_nan_aware(a, (c["feat"], c["npatch"], c["tlbr"]), c["name"] + " (batch)")
        for u, v in zip(a, b):
            assert torch.equal(u, v), f"{c['name']}: the batch entry point differs from a one-video call"


@pytest.mark.parametrize("kind", ["static", "allmerge"])
def test_full_length_static_and_all_merge(kind):
    """T = 128: chains of 128 nodes per cell, groups of 2048 patches.  Too large for a fixture: the referee is the oracle."""
    from oracle import sttm_oracle as O
    from sttm_amd import get_quadtree_features
    from sttm_amd.synth import synth_video
    if kind == "static":
        x = synth_video(1, 64, 14, 14, seed=5).expand(128, -1, -1, -1).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    else:
        x = D.allmerge_video(128, torch.float32)
    exp = O.get_quadtree_features(x, 0.85, 0.55, 1)
    if kind == "allmerge":
        assert exp[2].shape[0] == 16 and int(exp[1].max()) == 2048
    else:
        assert int(exp[1].sum()) == 128 * 196 and exp[2].shape[0] < 196
    D.check_nan_aware(get_quadtree_features(x.to(_dev()), 0.85, 0.55, 1), exp, f"T=128 {kind}")


# ----------------------------------------------------------------------------------------------
# 3. heavy-tailed, massive-activation family
# ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", D.HEAVY_COMBOS, ids=lambda c: "C%d_%s_%s_%s" % c)
@pytest.mark.parametrize("setting", D.HEAVY_SETTINGS)
def test_heavy_family_against_oracle(setting, combo):
    """A video whose every decision lies outside the band must be index-exact with features within the bars (the CPU test caps how
    many videos of a setting may fall outside that class at 10 %); in any other video every differing node traces to a decision
    inside the band."""
    from sttm_amd import get_quadtree_features
    C, dname, thr, tthr = combo
    for seed in D.HEAVY_SEEDS:
        x, m = D.heavy_case(setting, C, dname, thr, tthr, seed)
        out = get_quadtree_features(x.to(_dev()), thr, tthr, 1)
        what = f"heavy {setting} C={C} {dname} {thr}/{tthr} seed {seed}"
        if m.decisive:
            D.check_nan_aware(out, m.out, what)
        else:
            n = m.assert_differences_trace_to_the_band(out[2], out[1], what)
            print(f"{what}: {m.band_boxes.shape[0]} decisions inside the band, {n} nodes differ from the oracle")
            if n == 0:
                D.check_nan_aware(out, m.out, what)


# ----------------------------------------------------------------------------------------------
# the octree baseline decides with the same division-free test
# ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", D.OCTREE_KINDS)
def test_octree_degenerate_clip_equals_the_reference(kind):
    """A 2x2x2 cube of identical tokens with +Inf in one channel (the reference's NaN similarity splits it), norms past fp32
    overflow (similarity 0: nothing stops), an all-zero cube, one NaN element: against the reference's own output
    (tests/golden/odoct_*.npz)."""
    from sttm_amd.octree_utils import get_octree_features
    x, feat = D.load_odoct(kind)
    D.check_features_nan_aware(get_octree_features(x.to(_dev()), D.OCTREE_THR, D.OCTREE_ROOT), feat, f"octree {kind}")
