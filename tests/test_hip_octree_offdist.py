"""GPU parity of the octree baseline away from synth-v1 (tests/_octree_offdist.py):

1. near-threshold ladders on even sides (leaf level on sides 4 / 8 / 16, the level above it on side 8) -- outside the band
   eps = 2 * max |sim_oracle_fp32 - sim_float64| every decision decoded from the device's rows equals the float64 decision;
2. degenerate clips on ODD sides (7-4-2 and 5-3-2: cells with missing slots, which compare against the cube's origin leaf) against
   the reference's own rows (tests/golden/odo_*.npz), at an ordinary threshold and at 0.0, -0.3, 1.0, 1.5;
3. every pack width, row tail, side, root level, scan boundary and grid-stride loop of the kernels against the oracle, on videos
   whose every decision lies outside the band (asserted by tests/test_octree_offdist_cpu.py), and the cached workspace reused across
   calls of different sizes.

Not covered: the grid-stride loops of k_oct_pool and k_oct_emit (they wrap beyond 16.7 M threads, a ~0.5 GB input)."""
import pytest
import torch

from tests import _octree_offdist as X
from tests import _offdist as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(x, thr, root=0):
    from sttm_amd.octree_utils import get_octree_features
    return get_octree_features(x.to(DEV), thr, root)


# ---- 1. ladders ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", X.LADDERS, ids=X.ladder_id)
def test_ladder(spec):
    lad = X.oct_ladder(*spec)
    out = _run(lad.x, lad.thr).cpu()
    got = lad.decode(out)                  # asserts: every row is the block mean or the part it stands for, the count is consistent
    ins = ~lad.outside
    print(f"{X.ladder_id(spec)}: eps {lad.eps:.2e}, {int(ins.sum())} of {ins.numel()} decisions in the band, in-band flips device/oracle "
          f"{int(((got != lad.want32) & ins).sum())}, device/float64 {int(((got != lad.want64) & ins).sum())}")
    lad.assert_outside_band(got, X.ladder_id(spec))
    if lad.dtype != torch.float32 and torch.equal(got, lad.want32):
        assert D.bits_equal_nan_aware(out, lad.m.out32), "16-bit rows are not bit-equal to the oracle's although no decision differs"


# ---- 2. degenerate clips on odd sides -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", X.deg_cases(), ids=X.deg_id)
def test_degenerate_clip_equals_the_reference(case):
    from sttm_amd import get_quadtree_features
    kind, side, thr = case
    e = X.deg_expect(case)
    out = _run(e.x, thr).cpu()
    if e.pinned:
        D.check_features_nan_aware(out, e.feat, X.deg_id(case), tol=D.FP32_TOL)
        return
    # threshold 1.0 on bit-identical parent / child rows: in the band by construction, the reference's rounding decided its count
    rem = get_quadtree_features(e.x[e.T - 1:].to(DEV), thr, -1.0, 0)[0].cpu()
    cube = out[:out.shape[0] - rem.shape[0]]
    assert torch.equal(out[cube.shape[0]:].view(torch.int32), rem.view(torch.int32))
    if e.enumerable:
        # few in-band cells (static clips): count, order and every other decision are the float64 traversal's
        k = e.check_open(cube, X.deg_id(case))
        print(f"{X.deg_id(case)}: {cube.shape[0]} cube rows + {rem.shape[0]} remainder rows, {k} of {e.n_open} in-band cells stopped; the "
              f"reference has {e.feat.shape[0]} rows in all; bounds [{e.n_min}, {e.n_max}]")
        return
    assert X.is_const_thr1(case)
    n = e.check_free(cube, X.deg_id(case))
    print(f"{X.deg_id(case)}: {n} cube rows + {rem.shape[0]} remainder rows; the reference has {e.feat.shape[0]} rows in all; "
          f"bounds [{e.n_min}, {e.n_max}]")
    token = e.x.permute(0, 2, 3, 1)[0, 0, 0]
    assert e.rows_are_cells_bitwise(cube), "a row is not bit-equal to a pooled mean of the constant token"
    assert float(((out - token).abs() / token.abs().clamp_min(1.0)).max()) <= D.FP32_TOL, "a row is not the constant token"
    assert X.root_count(e.T, side) <= out.shape[0] <= e.feat.shape[0]


# ---- 3. dispatch and shape edges ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", X.PACK_CASES + X.TAIL_CASES, ids=X.case_id)
def test_pack_widths_and_row_tails(spec):
    c = X.case(*spec)
    X.check_rows(_run(c.x, c.thr, c.root), c.exp, X.case_id(spec))


def test_inputs_the_wrapper_has_to_copy():
    """A float32 channels-last view that starts 4 bytes into its storage, and an NCHW-contiguous input."""
    from sttm_amd.octree_utils import get_octree_features
    c = X.case(*X.PACK_CASES[2])                                         # fp32 C = 12
    T, C, H, W = c.x.shape
    flat = torch.empty(T * H * W * C + 1, device=DEV)
    flat[1:] = c.x.permute(0, 2, 3, 1).reshape(-1).to(DEV)
    view = flat[1:].view(T, H, W, C).permute(0, 3, 1, 2)
    assert view.data_ptr() % 16 == 4 and view.permute(0, 2, 3, 1).is_contiguous()
    X.check_rows(get_octree_features(view, c.thr, c.root), c.exp, "offset view")
    nchw = c.x.to(DEV).contiguous()
    assert nchw.is_contiguous() and not nchw.permute(0, 2, 3, 1).is_contiguous()
    X.check_rows(get_octree_features(nchw, c.thr, c.root), c.exp, "NCHW-contiguous")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16_bit_odd_channel_count_is_rejected(dtype):
    x = X.make_video("smooth", 5, 7, 5, 1, dtype)
    with pytest.raises(NotImplementedError, match="even channel count"):
        _run(x, 0.8)


@pytest.mark.parametrize("spec", X.SIDE_CASES, ids=X.case_id)
def test_sides_and_root_levels(spec):
    c = X.case(*spec)
    X.check_rows(_run(c.x, c.thr, spec[6]), c.exp, X.case_id(spec))


@pytest.mark.parametrize("side", X.SIDES)
def test_root_level_out_of_range_raises_index_error(side):
    from oracle import octree_oracle as OC
    n = len(OC.side_levels(side))
    x = X.case(*[s for s in X.SIDE_CASES if s[3] == side][0]).x
    for r in (n, -n - 1):
        with pytest.raises(IndexError):
            _run(x, 0.8, r)


@pytest.mark.parametrize("spec", X.SCAN_CASES, ids=X.case_id)
def test_scan_boundaries(spec):
    """4096 * k leaves: every scan workgroup is full.  At 2.0 every leaf is marked (the last included), at -2.0 only the roots are
    (the last leaf is not): values, not only counts."""
    c = X.case(*spec)
    out = _run(c.x, c.thr, c.root)
    k = c.x.shape[0] // 16
    if c.thr == 2.0:
        assert out.shape[0] == 4096 * k + 256
    elif c.thr == -2.0:
        assert out.shape[0] == 8 * k + 4
    X.check_rows(out, c.exp, X.case_id(spec))


def test_grid_stride_loops():
    """262 738 side-7 cells (one wave each, 262 144 per pass of k_oct_stop) and 2.1 M leaves (eight passes of k_oct_gather)."""
    c = X.case(*X.GRID_CASE)
    out = _run(c.x, c.thr, c.root)
    X.check_rows(out, c.exp, "grid-stride")


def test_workspace_reuse_across_sizes():
    """One stream: a large call, a small one in the same (cached) workspace, the large one again."""
    big, small = X.case(*X.WS_BIG), X.case(*X.WS_SMALL)
    xb, xs = big.x.to(DEV), small.x.to(DEV)
    a = _run(xb, big.thr)
    s = _run(xs, small.thr)
    b = _run(xb, big.thr)
    s2 = _run(xs, small.thr)
    X.check_rows(s, small.exp, "small after large")
    X.check_rows(a, big.exp, "large")
    assert torch.equal(a, b), "the large call's result changed after a small call in the same workspace"
    assert torch.equal(s, s2)
