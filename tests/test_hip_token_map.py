"""GPU: sttm_quadtree_token_map and the Python surface on top of them (get_quadtree_features_with_map,
unmerge_tokens, vis_flag=True).  Referee of the maps: tests/_token_map_ref.py (the CPU oracle's node list and representatives);
of the dictionaries: the reference's own, tests/golden/vis_*.npz, and the same helper on the shapes that have no fixture.  Small
shapes, chosen so that every path of the two kernels runs: 1 x 1 and many-leaf boxes, frames of more than one 1024-row scan
chunk, a clip of one frame, representatives in earlier frames."""
import os

import pytest
import torch

from tests._token_map_ref import VIS_GOLDEN, load_vis_case, ref_token_maps

pytestmark = pytest.mark.gpu
_ref_cache = {}


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _ref(key, x, args):
    """The helper's maps for one input, computed once and left unchanged."""
    if key not in _ref_cache:
        _ref_cache[key] = ref_token_maps(x, *args)
    return _ref_cache[key]


def _same_bits(a, b, what):
    for u, v, name in zip(a, b, ("features", "num_patches", "tlbr")):
        assert u.shape == v.shape and u.dtype == v.dtype and torch.equal(u, v), f"{what}: {name} differ"


def _check_maps(x, args, ref, what, vis=True, expect_dict=None):
    """The four checks of a case: maps == helper's, first three results == get_quadtree_features', bincount == num_patches, and the
    vis_flag=True call (dictionary + first three results)."""
    import sttm_amd
    xd = x.to(_dev())
    plain = sttm_amd.get_quadtree_features(xd, *args)
    feat, npatch, tlbr, t2o, t2n = sttm_amd.get_quadtree_features_with_map(xd, *args)
    T, _, H, W = x.shape
    assert t2o.shape == (T, H, W) and t2n.shape == (T, H, W) and t2o.dtype == torch.int32 and t2n.dtype == torch.int32
    assert torch.equal(t2o.cpu(), ref["token_to_out"]), f"{what}: token_to_out differs from the helper's"
    assert torch.equal(t2n.cpu(), ref["token_to_node"]), f"{what}: token_to_node differs from the helper's"
    _same_bits((feat, npatch, tlbr), plain, what)
    assert torch.equal(tlbr.cpu(), ref["tlbr"]), f"{what}: tlbr differs from the oracle's"
    assert torch.equal(torch.bincount(t2o.flatten().long(), minlength=npatch.shape[0]), npatch.long()), f"{what}: bincount != num_patches"
    if vis:
        out = sttm_amd.get_quadtree_features(xd, args[0], args[1], args[2], args[3], True)
        assert len(out) == 4
        want = ref["node_metadata"] if expect_dict is None else expect_dict
        assert out[3] == want and list(out[3]) == list(want), f"{what}: node_metadata differs"
        _same_bits(out[:3], sttm_amd.get_quadtree_features(xd, *args[:4]), what + " (vis_flag)")
    return feat, npatch, tlbr, t2o, t2n


@pytest.mark.parametrize("path", VIS_GOLDEN, ids=lambda p: os.path.basename(p)[:-4])
def test_golden_shapes_fp32(path):
    g = load_vis_case(path)
    ref = _ref(path, g["x"], g["args"])
    assert ref["node_metadata"] == g["node_metadata"]
    _check_maps(g["x"], g["args"], ref, g["name"], expect_dict=g["node_metadata"])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_sixteen_bit_rows(dtype):
    from sttm_amd.synth import synth_video
    x = synth_video(4, 64, 14, 14, seed=510, dtype=dtype)
    args = (0.85, 0.55, 1, False)
    _check_maps(x, args, _ref(("16", dtype), x, args), str(dtype))


def test_single_frame_has_no_pairs():
    from sttm_amd.synth import synth_video
    x = synth_video(1, 32, 14, 14, seed=511)
    args = (0.85, 0.55, 1, False)
    ref = _ref("T1", x, args)
    assert all(len(v) == 1 for v in ref["node_metadata"].values())
    _check_maps(x, args, ref, "T=1")


def test_identity_labels_without_the_temporal_stage():
    from sttm_amd.synth import synth_video
    x = synth_video(3, 32, 14, 14, seed=512)
    args = (0.85, -1.0, 1, False)
    _, _, tlbr, t2o, t2n = _check_maps(x, args, _ref("sp", x, args), "temporal_thresh=-1", vis=False)
    # every node is its own group: a token's node is the origin of its output row
    tl = tlbr.long()
    origin = (tl[:, 0] * 14 + tl[:, 1]) * 14 + tl[:, 2]
    assert torch.equal(origin[t2o.flatten().long()], t2n.flatten().long())
    import sttm_amd
    with pytest.raises(AssertionError):
        sttm_amd.get_quadtree_features(x.to(_dev()), 0.85, -1.0, 1, False, True)


def test_frames_of_more_than_one_scan_chunk():
    """H * W = 1360 rows per frame (two 1024-row chunks of the survivor scan), a 5-level tree."""
    from sttm_amd.synth import synth_video
    x = synth_video(2, 16, 34, 40, seed=513)
    args = (0.85, 0.55, 1, False)
    _check_maps(x, args, _ref("34x40", x, args), "34x40")


def test_forced_channel_tiled_spatial_stage():
    from sttm_amd import _lib
    from sttm_amd.synth import synth_video
    x = synth_video(8, 1024, 14, 14, seed=356)          # a case of test_forced_tiled_form_equals_one_workgroup_form
    args = (0.85, 0.55, 2, False)
    ref = _ref("tiled", x, args)
    try:
        _lib.configure(wide_lanes=256)
        _check_maps(x, args, ref, "wide_lanes=256")
    finally:
        _lib.configure(wide_lanes=0)


def test_map_belongs_to_the_last_merge_on_the_stream():
    import sttm_amd
    from sttm_amd.synth import synth_video
    xa, xb = synth_video(4, 32, 14, 14, seed=514), synth_video(4, 32, 14, 14, seed=515)
    args = (0.85, 0.55, 1, False)
    ra, rb = _ref("a", xa, args), _ref("b", xb, args)
    assert not torch.equal(ra["token_to_out"], rb["token_to_out"])
    da, db = xa.to(_dev()), xb.to(_dev())
    sttm_amd.get_quadtree_features(da, *args)
    out = sttm_amd.get_quadtree_features_with_map(db, *args)
    assert torch.equal(out[3].cpu(), rb["token_to_out"]) and torch.equal(out[4].cpu(), rb["token_to_node"])
    out = sttm_amd.get_quadtree_features_with_map(da, *args)
    assert torch.equal(out[3].cpu(), ra["token_to_out"]) and torch.equal(out[4].cpu(), ra["token_to_node"])


def test_vis_flag_ignores_slow_ver_and_head_dim():
    import sttm_amd
    g = load_vis_case(VIS_GOLDEN[0])
    xd = g["x"].to(_dev())
    thr, tthr, root, w = g["args"]
    a = sttm_amd.get_quadtree_features(xd, thr, tthr, root, w, True)
    b = sttm_amd.get_quadtree_features(xd, thr, tthr, root, w, True, slow_ver=True, head_dim=16)
    _same_bits(b[:3], a[:3], "slow_ver / head_dim")
    assert a[3] == b[3] == g["node_metadata"]


def test_default_call_issues_no_map(monkeypatch):
    """Without want_map the library's map entry point is not called at all; with it, once per merge."""
    from sttm_amd import quadtree_interface as Q
    g = load_vis_case(VIS_GOLDEN[0])
    thr, tthr, root, w = g["args"]
    xd = g["x"].to(_dev())
    real, calls = Q._token_map, []

    def spy(ctx, root_level):
        calls.append(root_level)
        return real(ctx, root_level)

    monkeypatch.setattr(Q, "_token_map", spy)
    assert len(Q.quadtree_merge_raw(xd, thr, tthr, root, w, None)) == 4
    assert calls == []
    out = Q.quadtree_merge_raw(xd, thr, tthr, root, w, None, want_map=True)
    assert len(out) == 5 and calls == [root]
    assert torch.equal(out[4][0].cpu(), _ref(VIS_GOLDEN[0], g["x"], g["args"])["token_to_out"])


def test_map_survives_the_barrier_retry(monkeypatch):
    """A grid-barrier timeout repeats the merge on the two-launch label path; the map is taken once, from the call that succeeded."""
    import sttm_amd
    from sttm_amd import quadtree_interface as Q
    g = load_vis_case(VIS_GOLDEN[0])
    ref = _ref(VIS_GOLDEN[0], g["x"], g["args"])
    xd = g["x"].to(_dev())
    plain = sttm_amd.get_quadtree_features(xd, *g["args"])
    real_merge, real_map, log = Q._merge_locked, Q._token_map, []

    def merge(st, *a, **k):
        flags = a[10]
        log.append(("merge", flags))
        if len(log) == 1:
            raise Q.BarrierTimeout("injected")
        return real_merge(st, *a, **k)

    def token_map(ctx, root_level):
        log.append(("map", None))
        return real_map(ctx, root_level)

    monkeypatch.setattr(Q, "_merge_locked", merge)
    monkeypatch.setattr(Q, "_token_map", token_map)
    st = Q._acquire_state(xd.device)
    left, st.no_fuse_left = st.no_fuse_left, 0
    st.lock.release()
    try:
        with pytest.warns(UserWarning, match="two-launch label path"):
            out = sttm_amd.get_quadtree_features_with_map(xd, *g["args"])
    finally:
        st.no_fuse_left = left                     # the injected timeout must not keep this stream off the fused path
    assert log == [("merge", 0), ("merge", Q.FLAG_NO_FUSE), ("map", None)]
    _same_bits(out[:3], plain, "after the retry")
    assert torch.equal(out[3].cpu(), ref["token_to_out"]) and torch.equal(out[4].cpu(), ref["token_to_node"])


# ---- unmerge_tokens ------------------------------------------------------------------------------------------------------

def _merged(T, C, dtype, seed):
    import sttm_amd
    from sttm_amd.synth import synth_video
    x = synth_video(T, C, 14, 14, seed=seed, dtype=dtype).to(_dev())
    out = sttm_amd.get_quadtree_features_with_map(x, 0.85, 0.55, 1, False)
    return out[0], out[3]


@pytest.mark.parametrize("T,C,dtype,keep", [(4, 32, torch.float32, None), (4, 64, torch.bfloat16, None), (4, 64, torch.float16, 20),
                                            (2, 1024, torch.float32, None)], ids=["f32_C32", "bf16_C64", "f16_C20_40_byte_rows", "f32_C1024"])
def test_unmerge_equals_indexing(T, C, dtype, keep):
    import sttm_amd
    feat, t2o = _merged(T, C, dtype, 520 + C)
    if keep:
        feat = feat[:, :keep].contiguous()              # 40-byte rows
    got = sttm_amd.unmerge_tokens(feat, t2o)
    want = feat[t2o.flatten().long()].reshape(T, 14, 14, feat.shape[1])
    assert got.shape == want.shape and got.dtype == feat.dtype and got.is_contiguous()
    assert torch.equal(got.view(torch.uint8), want.contiguous().view(torch.uint8))


def test_unmerge_into_a_callers_tensor():
    import sttm_amd
    feat, t2o = _merged(4, 32, torch.float32, 530)
    dest = torch.full((4, 14, 14, 32), 7.0, device=_dev())
    got = sttm_amd.unmerge_tokens(feat, t2o, out=dest)
    assert got.data_ptr() == dest.data_ptr()
    assert torch.equal(dest, feat[t2o.flatten().long()].reshape(4, 14, 14, 32))
    with pytest.raises(ValueError):
        sttm_amd.unmerge_tokens(feat, t2o, out=torch.empty((4, 14, 14, 31), device=_dev()))


def test_unmerge_refuses_cpu_tensors():
    import sttm_amd
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sttm_amd.unmerge_tokens(torch.zeros(3, 4), torch.zeros(1, 2, 2, dtype=torch.int32))
