"""GPU parity of the upstream pooling kernels away from unit-variance Gaussians (tests/_pool_offdist.py): get_2dPool, resize_nearest
and the pooling fused into the spatial kernel's leaf load on inputs with NaN / +Inf / -Inf in the first, an interior and the last
window and in the dropped row / column, a zero frame, and scalings by 2^62 and 2^-70 -- against what the reference's get_2dPool
returned (tests/golden/poolod_*.npz) and against the oracle.  Max pooling follows ATen's rule `(val > maxval) || isnan(val)`: a NaN
in a window reaches the output."""
import pytest
import torch

from tests import _pool_offdist as PD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("case", PD.cases(), ids=PD.case_id)
def test_pool_off_distribution_equals_the_reference(case):
    """All three modes on one fixture: the reference's NaN / Inf pattern and finite values within the existing bars; bit-identical to
    the oracle (same arithmetic order), non-finite values included."""
    from oracle import pool_oracle as P
    from sttm_amd.upstream import get_2dPool
    kind, side, stride, dname = case
    x, ys = PD.load(case)
    for mode in PD.MODES:
        what = f"{PD.case_id(case)} {mode}"
        out = get_2dPool(x.to(DEV), stride=stride, width=side, mode=mode).cpu()
        PD.close_to_reference(out, ys[mode], mode, stride, what)
        assert PD.bits_equal(out, P.get_2dpool(x, stride, side, side, mode)), f"{what}: not bit-identical to the oracle"


@pytest.mark.parametrize("case", PD.cases(("float16",)), ids=PD.case_id)
def test_pool_off_distribution_float16_against_oracle(case):
    from oracle import pool_oracle as P
    from sttm_amd.upstream import get_2dPool
    kind, side, stride, dname = case
    x = PD.build(kind, side, stride, torch.float16)
    for mode in PD.MODES:
        out = get_2dPool(x.to(DEV), stride=stride, width=side, mode=mode).cpu()
        exp = P.get_2dpool(x, stride, side, side, mode)
        PD.same_nonfinite(out, exp, f"{PD.case_id(case)} {mode}")
        assert PD.bits_equal(out, exp), f"{PD.case_id(case)} {mode}: not bit-identical to the oracle"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("stride,C", [(2, 8), (3, 7), (4, 6), (2, 1030)])
def test_max_pool_propagates_nan_from_every_window_slot(stride, C, dtype):
    """One NaN per window, in window w at slot w mod stride^2, each in another channel: every window's output is NaN in that channel
    and nowhere else (F.max_pool2d's behaviour; the oracle restates ATen's rule).  C = 1030 makes the 16-bit rows loop (more than 512
    packs of 2); odd C runs the fp32 scalar packs."""
    from oracle import pool_oracle as P
    from sttm_amd.upstream import get_2dPool
    if dtype != torch.float32 and C % 2:
        C += 1
    n = 5
    side = n * stride + (1 if stride > 2 else 0)
    g = torch.Generator().manual_seed(stride * 100 + C)
    x = torch.randn(2, side, side, C, generator=g)
    want = torch.zeros(2, n, n, C, dtype=torch.bool)
    for t in range(2):
        for oy in range(n):
            for ox in range(n):
                w = (t * n + oy) * n + ox
                slot, ch = w % (stride * stride), (3 * w) % C
                x[t, oy * stride + slot // stride, ox * stride + slot % stride, ch] = float("nan")
                want[t, oy, ox, ch] = True
    x = x.reshape(2, side * side, C).to(dtype)
    out = get_2dPool(x.to(DEV), stride=stride, width=side, mode="max").cpu()
    assert torch.equal(torch.isnan(out.float()).reshape(2, n, n, C), want)
    assert PD.bits_equal(out, P.get_2dpool(x, stride, side, side, "max"))


@pytest.mark.parametrize("case", PD.cases(PD.FIXTURE_DTYPES + ("float16",)), ids=PD.case_id)
def test_resize_nearest_off_distribution_is_a_bit_exact_gather(case):
    from oracle import pool_oracle as P
    from sttm_amd.upstream import resize_nearest
    kind, side, stride, dname = case
    x = PD.build(kind, side, stride, PD.DTYPES[dname])
    for tgt in ((side + 1) // 2, side + 3):
        out = resize_nearest(x.to(DEV), side, side, (tgt, tgt)).cpu()
        assert PD.bits_equal(out, P.resize_nearest(x, side, side, (tgt, tgt))), f"{PD.case_id(case)} -> {tgt}"


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


@pytest.mark.parametrize("mode", PD.MODES)
@pytest.mark.parametrize("case", PD.cases(PD.FIXTURE_DTYPES + ("float16",)), ids=PD.case_id)
def test_fused_pool_off_distribution(case, mode):
    """The pool fused into the leaf load (force_fused=True; 3 x 3 windows take the two steps on the device) against
    pool_oracle o sttm_oracle -- same nodes, NaN / Inf at the same places, finite features within the bars -- and bit-identical,
    NaN payloads included, to the device's own pool-then-merge."""
    from oracle import pool_oracle as P
    from oracle import sttm_oracle as O
    from sttm_amd import get_quadtree_features, get_quadtree_features_from_pooled_input
    from sttm_amd.upstream import get_2dPool
    from tests import _offdist as D
    kind, side, stride, dname = case
    x = PD.build(kind, side, stride, PD.DTYPES[dname])
    pooled = P.get_2dpool(x, stride, side, side, mode)
    hw = int(round(pooled.shape[1] ** 0.5))
    root = 0 if hw == 8 else 1                                       # 8-4-2 / 14-7-4 / 13-7-4: three levels
    vid = lambda p: p.reshape(PD.T, hw, hw, PD.C).permute(0, 3, 1, 2)          # noqa: E731
    exp = O.get_quadtree_features(vid(pooled), 0.85, 0.55, root)
    out = get_quadtree_features_from_pooled_input(x.to(DEV), 0.85, 0.55, root, stride=stride, mode=mode, width=side, force_fused=True)
    D.check_nan_aware(out, exp, f"{PD.case_id(case)} {mode} fused")
    two = get_quadtree_features(vid(get_2dPool(x.to(DEV), stride=stride, width=side, mode=mode)), 0.85, 0.55, root)
    assert torch.equal(out[2], two[2]) and torch.equal(out[1], two[1])
    assert torch.equal(_bits(out[0]), _bits(two[0])), "the fused features are not bit-identical to pool-then-merge"
