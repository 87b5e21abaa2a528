"""GPU: token rows wider than one workgroup (more than 1024 channel packs: fp32 C > 4096, 16-bit C > 8192) run the channel-tiled
spatial stage (csrc/spatial_wide.inc).  Referee: the CPU oracle, with test_hip_parity.py's bar (indices exact, features within
tolerance).  The tiled form forced onto rows that fit one workgroup (sttm_configure "wide_lanes") must give the one-workgroup form's
node set and feature bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-5
BF16_TOL = 2 ** -7


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _check(out, exp, tol, what=""):
    feat, npatch, tlbr = out[:3]
    efeat, enpatch, etlbr = exp[:3]
    tl, np_, ft = tlbr.cpu(), npatch.cpu(), feat.cpu()
    assert tl.shape == etlbr.shape, f"{what}: N'={tl.shape[0]} expected {etlbr.shape[0]}"
    if not torch.equal(tl, etlbr):
        bad = (tl != etlbr).any(dim=1).nonzero().flatten()
        raise AssertionError(f"{what}: tlbr differs at rows {bad[:5].tolist()}: {tl[bad[0]].tolist()} vs {etlbr[bad[0]].tolist()}")
    assert torch.equal(np_, enpatch), f"{what}: num_patches differ"
    err = (ft.float() - efeat.float()).abs()
    scale = efeat.float().abs().clamp_min(1.0) if feat.dtype != torch.float32 else 1.0
    worst = float((err / scale).max()) if err.numel() else 0.0
    assert worst <= tol, f"{what}: feature max err {worst:.3e} > {tol:.1e}"


def _identical(a, b, what):
    for u, v, name in zip(a, b, ("features", "num_patches", "tlbr", "extra")):
        assert u.shape == v.shape and torch.equal(u, v), f"{what}: {name} differ"


def test_fp32_8192_wide_row_matches_oracle():
    """The row the issue is about: a 72B hidden state in float32 (8192 channels = 2048 16-byte packs)."""
    from oracle import sttm_oracle as O
    from sttm_amd import get_quadtree_features
    from sttm_amd.synth import synth_video
    x = synth_video(6, 8192, 14, 14, seed=300)
    exp = O.get_quadtree_features(x, 0.85, 0.55, 1, False)
    _check(get_quadtree_features(x.to(_dev()), 0.85, 0.55, 1, False), exp, FP32_TOL, "fp32 C=8192")


WIDE_CASES = [
    # (T, C, H, W, seed, dtype, threshold, temporal, root_level, keyword arguments)
    (4, 4100, 14, 14, 301, torch.float32, 0.85, 0.55, 1, {}),          # 1025 lanes: two chunks
    (4, 5000, 14, 14, 302, torch.float32, 0.85, 0.55, 1, {}),
    (4, 6144, 14, 14, 303, torch.float32, 0.85, 0.55, 1, {}),
    (4, 4098, 14, 14, 304, torch.float32, 0.85, 0.55, 1, {}),          # 2-wide packs
    (3, 4097, 14, 14, 305, torch.float32, 0.85, 0.55, 1, {}),          # scalar packs: five chunks
    (4, 8200, 14, 14, 306, torch.bfloat16, 0.85, 0.55, 1, {}),
    (3, 12288, 14, 14, 307, torch.bfloat16, 0.85, 0.55, 1, {}),
    (3, 16384, 14, 14, 308, torch.bfloat16, 0.85, 0.55, 1, {}),
    (4, 8200, 14, 14, 309, torch.float16, 0.85, 0.55, 1, {}),
    (3, 12288, 14, 14, 310, torch.float16, 0.85, 0.55, 1, {}),
    (3, 16384, 14, 14, 311, torch.float16, 0.85, 0.55, 1, {}),
    (3, 8192, 20, 36, 312, torch.float32, 0.85, 0.60, 1, {}),          # 4-level tree (Qwen2-VL grid)
    (3, 8192, 18, 26, 313, torch.float32, 0.85, 0.60, 1, {}),
    (3, 8192, 13, 24, 314, torch.float32, 0.85, 0.60, 1, {}),
    (3, 16384, 20, 36, 315, torch.bfloat16, 0.85, 0.60, 1, {}),
    (4, 8192, 14, 14, 316, torch.float32, 0.85, 0.55, -1, {}),         # no pyramid
    (4, 8192, 14, 14, 317, torch.float32, 0.85, 0.55, 0, {}),          # 4-level tree at root 0
    (4, 8192, 14, 14, 318, torch.float32, 0.85, 0.55, 2, {}),          # 2-level tree
    (4, 8192, 14, 14, 319, torch.float32, 0.85, 0.55, 1, dict(weighted_avg=True)),
    (4, 8192, 14, 14, 320, torch.float32, 0.85, 0.55, 1, dict(slow_ver=True)),
    (4, 8192, 14, 14, 321, torch.float32, 0.85, 0.55, 1, dict(head_dim=128)),
    (3, 8192, 20, 36, 322, torch.float32, 0.85, 0.60, 1, dict(head_dim=128)),
    (4, 16384, 14, 14, 323, torch.bfloat16, 0.85, 0.55, 1, dict(head_dim=128)),
    (4, 8192, 14, 14, 324, torch.float32, 0.85, -1.0, 1, {}),          # temporal stage off
    (4, 8192, 14, 14, 325, torch.float32, 0.70, 0.50, 1, dict(synth=dict(c=0.05, p_static=0.9))),    # smooth: nodes at every level
    (3, 8192, 20, 36, 326, torch.float32, 0.70, 0.50, 1, dict(synth=dict(c=0.05, p_static=0.9))),
]


@pytest.mark.parametrize("case", WIDE_CASES, ids=lambda c: "T%d_C%d_%dx%d_s%d_r%d" % (c[:5] + (c[8],)))
def test_wide_rows_against_oracle(case):
    from oracle import sttm_oracle as O
    from sttm_amd import get_quadtree_features
    from sttm_amd.synth import synth_video
    T, C, H, W, seed, dtype, thr, tthr, root, kw = case
    kw = dict(kw)
    x = synth_video(T, C, H, W, seed=seed, dtype=dtype, **kw.pop("synth", {}))
    weighted = kw.pop("weighted_avg", False)
    exp = O.get_quadtree_features(x, thr, tthr, root, weighted, **kw)
    out = get_quadtree_features(x.to(_dev()), thr, tthr, root, weighted, **kw)
    _check(out, exp, FP32_TOL if dtype == torch.float32 else BF16_TOL, str(case[:5]))


@pytest.mark.parametrize("pe_weighted", [False, True])
def test_wide_rows_with_position_embeddings(pe_weighted):
    """sttm_quadtree_apply after a tiled merge: the side tensors are pooled over the nodes / groups the tiled stage decided."""
    from oracle import sttm_oracle as O
    from sttm_amd import get_quadtree_features
    from sttm_amd.synth import synth_video
    x = synth_video(4, 8192, 14, 14, seed=330)
    pe = (synth_video(4, 128, 14, 14, seed=331), synth_video(4, 128, 14, 14, seed=332))
    exp = O.get_quadtree_features(x, 0.85, 0.55, 1, False, pos_embs=pe, pos_emb_weighted_avg=pe_weighted)
    out = get_quadtree_features(x.to(_dev()), 0.85, 0.55, 1, False, pos_embs=tuple(p.to(_dev()) for p in pe),
                                pos_emb_weighted_avg=pe_weighted)
    _check(out[:3], exp[:3], FP32_TOL, "pos_embs")
    for got, want in zip(out[3], exp[3]):
        assert got.shape == want.shape
        assert float((got.cpu() - want).abs().max()) <= FP32_TOL


FULL_LENGTH = [
    (128, 8192, 14, 14, 340, 0.85, 0.55),      # Video-MME preset
    (180, 8192, 14, 14, 341, 0.94, 0.82),      # MLVU preset
]


@pytest.mark.parametrize("case", FULL_LENGTH, ids=lambda c: "T%d_C%d" % c[:2])
def test_wide_rows_full_length(case):
    from oracle import sttm_oracle as O
    from sttm_amd import get_quadtree_features
    from sttm_amd.synth import synth_video
    T, C, H, W, seed, thr, tthr = case
    x = synth_video(T, C, H, W, seed=seed)
    exp = O.get_quadtree_features(x, thr, tthr, 1, False)
    _check(get_quadtree_features(x.to(_dev()), thr, tthr, 1, False), exp, FP32_TOL, str(case[:2]))


FORCED = [
    # (T, C, H, W, seed, dtype, threshold, temporal, root_level)
    (8, 1024, 14, 14, 350, torch.float32, 0.85, 0.55, 1),
    (8, 4096, 14, 14, 351, torch.float32, 0.85, 0.55, 1),
    (6, 1024, 20, 36, 352, torch.float32, 0.85, 0.60, 1),
    (6, 4096, 20, 36, 353, torch.float32, 0.85, 0.60, 1),
    (8, 3584, 14, 14, 354, torch.bfloat16, 0.85, 0.55, 1),
    (6, 3584, 20, 36, 355, torch.bfloat16, 0.85, 0.60, 1),
    (8, 1024, 14, 14, 356, torch.float32, 0.85, 0.55, 2),
    (8, 1024, 14, 14, 357, torch.float32, 0.85, 0.55, 0),
    (8, 1024, 14, 14, 358, torch.float32, 0.70, 0.50, 1),
]


@pytest.mark.parametrize("lanes", [256, 512])
@pytest.mark.parametrize("case", FORCED, ids=lambda c: "T%d_C%d_%dx%d_s%d_r%d" % (c[:5] + (c[8],)))
def test_forced_tiled_form_equals_one_workgroup_form(case, lanes):
    """wide_lanes = 256 / 512 runs the tiled stage on rows that fit one workgroup: node set, merged-token indices and feature bits
    equal the default path's (only the summation order of the statistics differs)."""
    from sttm_amd import _lib
    from sttm_amd.quadtree_interface import get_quadtree_features_into
    from sttm_amd.synth import synth_video
    T, C, H, W, seed, dtype, thr, tthr, root = case
    x = synth_video(T, C, H, W, seed=seed, dtype=dtype).to(_dev())
    outs = []
    try:
        for wl in (0, lanes):
            _lib.configure(wide_lanes=wl)
            dest = torch.empty((T * H * W, C), dtype=dtype, device=_dev())
            outs.append([o.clone() for o in get_quadtree_features_into(dest, x, thr, tthr, root, False, return_idx=True)])
    finally:
        _lib.configure(wide_lanes=0)
    _identical(outs[1], outs[0], f"wide_lanes={lanes}")


def test_batch_equals_one_call_per_video():
    from sttm_amd import get_quadtree_features
    from sttm_amd.quadtree_interface import get_quadtree_features_batch
    from sttm_amd.synth import synth_video
    for C, dtype, H, W in ((8192, torch.float32, 14, 14), (16384, torch.bfloat16, 14, 14), (8192, torch.float32, 20, 36)):
        xs = [synth_video(4, C, H, W, seed=360 + i, dtype=dtype).to(_dev()) for i in range(3)]
        singles = [get_quadtree_features(x, 0.85, 0.55, 1, False) for x in xs]
        batch = get_quadtree_features_batch(xs, 0.85, 0.55, 1, False)
        for s, b in zip(singles, batch):
            _identical(b, s, f"batch C={C}")


def test_into_on_a_hidden_state_window():
    """The hook's fused slice -> merge -> concat on a [1, S, 8192] float32 hidden state."""
    from oracle import sttm_oracle as O
    from sttm_amd.quadtree_interface import get_quadtree_features_into
    T, H, W, C = 4, 14, 14, 8192
    from sttm_amd.synth import synth_video
    vid = synth_video(T, C, H, W, seed=370)                                  # [T, C, H, W]
    pre, post = 13, 7
    S = pre + T * H * W + post
    hidden = torch.randn(1, S, C, generator=torch.Generator().manual_seed(371))
    hidden[0, pre:pre + T * H * W] = vid.permute(0, 2, 3, 1).reshape(T * H * W, C)
    hidden = hidden.to(_dev())
    view = hidden[0, pre:pre + T * H * W].view(T, H, W, C).permute(0, 3, 1, 2)
    new = torch.zeros(S, C, device=_dev())
    feat, npatch, tlbr, idx = get_quadtree_features_into(new[pre:], view, 0.85, 0.55, 1, False, return_idx=True)
    exp = O.get_quadtree_features(vid, 0.85, 0.55, 1, False)
    _check((feat, npatch, tlbr), exp, FP32_TOL, "into")
    want_idx = exp[2][:, 0] * H * W + exp[2][:, 1] * W + exp[2][:, 2]
    assert torch.equal(idx.cpu().long(), want_idx.long())
    assert torch.equal(new[:pre].cpu(), torch.zeros(pre, C)), "rows before the window were written"


def test_pooled_input_takes_the_two_step_path():
    from sttm_amd import get_quadtree_features
    from sttm_amd.quadtree_interface import get_quadtree_features_from_pooled_input
    from sttm_amd.upstream import get_2dPool
    T, C = 3, 8192
    g = torch.Generator().manual_seed(380)
    x = torch.randn(T, 729, C, generator=g).to(_dev())
    out = get_quadtree_features_from_pooled_input(x, 0.85, 0.55, 1, False)
    pooled = get_2dPool(x, stride=2, width=27, mode="bilinear")
    exp = get_quadtree_features(pooled.reshape(T, 14, 14, C).permute(0, 3, 1, 2), 0.85, 0.55, 1, False)
    _identical(out, exp, "pooled input")


def test_stand_alone_temporal_stage_on_wide_nodes():
    from oracle import sttm_oracle as O
    from sttm_amd.quadtree_interface import cross_frame_node_merging_fast
    from sttm_amd.synth import synth_video
    T, C, H, W = 4, 8192, 14, 14
    x = synth_video(T, C, H, W, seed=390)
    nf, nn, nt = O.get_quadtree_features(x, 0.85, -1.0, 1, False)
    exp = O.temporal_merge(nf, nt, nn, 0.55, False, None, False)
    res = cross_frame_node_merging_fast(nf.to(_dev()), nt.to(_dev()), 0.55, nn.to(_dev()), False, None, grid=(T, H, W), root_level=1)
    _check((res["feature"], res["num_patch"], res["tlbr"]), exp[:3], FP32_TOL, "nodes")


def test_deep_trees_with_wide_rows_stay_fenced():
    from sttm_amd import get_quadtree_features
    from sttm_amd.synth import synth_video
    x = synth_video(1, 8192, 27, 27, seed=395).to(_dev())                   # 5 levels at root_level 0
    with pytest.raises(NotImplementedError, match="at most 4 levels"):
        get_quadtree_features(x, 0.85, 0.55, 0, False)
