"""CPU side of the pooling off-distribution tests (tests/_pool_offdist.py): every fixture is bit-equal to its builder, holds what its
name says, and the oracle (oracle/pool_oracle.py) reproduces what the reference's get_2dPool returned on it -- NaN, +Inf and -Inf at
identical positions, finite values within tests/_golden.pool_close_enough's bars."""
import glob
import os

import pytest
import torch

from oracle import pool_oracle as P
from tests import _pool_offdist as PD
from tests._golden import GOLDEN_DIR, POOL_GOLDEN


def test_fixture_list_is_the_case_table():
    have = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "poolod_*.npz")))
    assert have == sorted(PD.fixture_name(c) for c in PD.cases())
    assert not any("poolod_" in p for p in POOL_GOLDEN)            # the on-distribution list (pool_*.npz) is unchanged
    for name in have:
        assert os.path.getsize(os.path.join(GOLDEN_DIR, name + ".npz")) < 256 * 1024


@pytest.mark.parametrize("case", PD.cases(), ids=PD.case_id)
def test_oracle_reproduces_the_reference_off_distribution(case):
    kind, side, stride, dname = case
    x, ys = PD.load(case)
    assert PD.bits_equal(x, PD.build(kind, side, stride, PD.DTYPES[dname])), "the fixture's input is not what the builder makes"
    for mode in PD.MODES:
        out = P.get_2dpool(x, stride, side, side, mode)
        PD.close_to_reference(out, ys[mode], mode, stride, f"{PD.case_id(case)} {mode}")


@pytest.mark.parametrize("dname", PD.FIXTURE_DTYPES)
@pytest.mark.parametrize("side,stride", PD.SHAPES)
def test_fixtures_hold_what_their_names_say(side, stride, dname):
    """The reference's max pooling propagates NaN (ATen: `(val > maxval) || isnan(val)`): both NaN windows come out NaN, the window
    with -Inf and +Inf is +Inf and the lone -Inf loses to a finite neighbour; the average of -Inf and +Inf is NaN; a NaN in the row
    the windows drop reaches no window output but reaches the bilinear one."""
    x, ys = PD.load(("nonfinite", side, stride, dname))
    n = side // stride
    mx, av, bl = (ys[m].float() for m in PD.MODES)
    g = mx.reshape(PD.T, n, n, PD.C)
    assert torch.isnan(g[0, 0, 0, 1]) and torch.isnan(g[1, n - 1, n - 1, 7]) and int(torch.isnan(mx).sum()) == 2
    assert g[0, n - 1, n - 1, 3] == float("inf") and g[0, n // 2, n // 2, 2] == float("inf") and g[1, 0, 0, 0] == float("inf")
    assert int(torch.isneginf(mx).sum()) == 0 and torch.isfinite(g[1, 2, 3, 1])
    a = av.reshape(PD.T, n, n, PD.C)
    assert torch.isnan(a[0, n - 1, n - 1, 3]) and torch.isnan(a[1, n // 2, n // 2, 6]) and a[1, 2, 3, 1] == float("-inf")
    if side % stride:
        assert int(torch.isnan(bl).sum()) > int(torch.isnan(av).sum())     # the dropped row's NaNs are bilinear taps
    z, zs = PD.load(("zero_frame", side, stride, dname))
    assert all(float(zs[m][1].float().abs().max()) == 0.0 for m in PD.MODES)
    for kind, lo, hi in (("scale_p62", 2.0 ** 55, 2.0 ** 66), ("scale_m70", 2.0 ** -77, 2.0 ** -66)):
        _, ss = PD.load((kind, side, stride, dname))
        assert all(lo < float(ss[m].float().abs().max()) < hi for m in PD.MODES)


def test_float16_inputs_saturate_as_the_device_test_expects():
    """float16 has no fixture: 2^62 takes every element to +-Inf and 2^-70 to zero; the oracle is the referee there."""
    assert bool(torch.isinf(PD.build("scale_p62", 24, 3, torch.float16).float()).all())
    assert float(PD.build("scale_m70", 24, 3, torch.float16).float().abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("stride", [2, 3])
def test_oracle_max_follows_aten_on_signed_zero_ties_and_nan(stride, dtype):
    """The oracle's max is ATen's rule in window order, `(val > maxval) || isnan(val)`: of -0.0 and +0.0 the FIRST one of the window
    stays (torch.equal cannot see that: the sign bits are compared), a NaN is returned, and a window of -Inf alone gives -Inf."""
    import torch.nn.functional as F
    side, C = 4 * stride, 6
    g = torch.Generator().manual_seed(stride)
    sign = torch.randint(0, 2, (2, side, side, C), generator=g).bool()
    x = torch.where(sign, torch.tensor(-0.0), torch.tensor(0.0))
    x[0, :stride, :stride, 0] = torch.randn(stride, stride, generator=g)          # an ordinary window
    x[0, 0, stride + 1, 1] = -1.0                                                  # zeros of both signs beat a negative value
    x[1, stride:2 * stride, :stride, 2] = float("-inf")                           # -Inf alone
    x[1, 2 * stride + 1, 2 * stride, 3] = float("nan")
    x = x.to(dtype)
    ref = F.max_pool2d(x.permute(0, 3, 1, 2).float(), stride).permute(0, 2, 3, 1).reshape(2, -1, C).to(dtype)
    out = P.get_2dpool(x.reshape(2, side * side, C), stride, side, side, "max")
    assert PD.bits_equal(out, ref)
    assert torch.equal(torch.signbit(out.float()), torch.signbit(ref.float()))
    zeros = out.float() == 0
    assert bool(torch.signbit(out.float())[zeros].any()) and bool((~torch.signbit(out.float()))[zeros].any()), "both zeros must occur"
