"""Off-distribution inputs for the upstream pooling kernels (get_2dPool, resize_nearest, the pooling fused into the spatial leaf load):
non-finite elements in the first, an interior and the last window and in the row / column that floor(side / stride) drops, a zero
frame, and scalings past fp32 overflow of a window sum (2^62 ... only the products of the merge stage overflow; the pooled values stay
finite) and below the cosine's eps clamp (2^-70).  Shared by tests/test_pool_offdist_cpu.py, tests/test_hip_pool_offdist.py and
tests/golden/make_golden_pool_offdist.py.  Everything here runs on the CPU."""
import functools
import json
import os

import numpy as np
import torch

from tests._golden import GOLDEN_DIR, _t

NAN, INF = float("nan"), float("inf")
T, C = 2, 8
SHAPES = ((27, 2), (28, 2), (24, 3))                    # (side, stride): 27 -> 14 (bilinear) / 13 (windows), 28 -> 14, 24 -> 8
MODES = ("max", "average", "bilinear")
KINDS = ("nonfinite", "zero_frame", "scale_p62", "scale_m70")
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
SHORT = {"float32": "f32", "bfloat16": "bf16", "float16": "f16"}
FIXTURE_DTYPES = ("float32", "bfloat16")               # float16 runs against the oracle only


def build(kind, side, stride, dtype):
    """[T, side*side, C] tokens"""
    g = torch.Generator().manual_seed(1000 * side + 10 * stride + KINDS.index(kind))
    x = torch.randn(T, side, side, C, generator=g)
    n = side // stride                                   # windows per axis of average / max
    mid, last = stride * (n // 2), stride * (n - 1)
    if kind == "nonfinite":
        x[0, 0, 0, 1] = NAN                              # first window
        x[0, mid + 1, mid, 2] = INF                      # an interior window
        x[0, last, last, 3] = -INF                       # -Inf and +Inf in the last window: max +Inf, average NaN
        x[0, last + 1, last + 1, 3] = INF
        x[1, 1, 1, 0] = INF
        x[1, mid, mid + 1, 6] = -INF
        x[1, mid + 1, mid, 6] = INF
        x[1, last + stride - 1, last, 7] = NAN           # last window
        x[1, 2 * stride, 3 * stride, 1] = -INF           # -Inf alone: a finite neighbour is the maximum
        if side % stride:                                # the row / column the windows never read (the bilinear taps do)
            x[0, side - 1, 5, 4] = NAN
            x[0, 7, side - 1, 5] = INF
            x[1, side - 1, side - 1, 2] = NAN
    elif kind == "zero_frame":
        x[1] = 0
    elif kind == "scale_p62":
        x = x * 2.0 ** 62
    elif kind == "scale_m70":
        x = x * 2.0 ** -70
    else:
        raise ValueError(kind)
    return x.reshape(T, side * side, C).to(dtype)


def cases(dtypes=FIXTURE_DTYPES):
    return [(k, side, stride, d) for k in KINDS for side, stride in SHAPES for d in dtypes]


def fixture_name(case):
    kind, side, stride, d = case
    return f"poolod_{kind}_{side}_s{stride}_{SHORT[d]}"


def case_id(case):
    return fixture_name(case)[7:]


@functools.lru_cache(maxsize=None)
def load(case):
    """tests/golden/poolod_*.npz -> (x, {mode: what the reference's get_2dPool returned})"""
    z = np.load(os.path.join(GOLDEN_DIR, fixture_name(case) + ".npz"))
    meta = json.loads(str(z["meta"]))
    return _t(z["x"], meta["dtype"]), {m: _t(z["y_" + m], meta["dtype"]) for m in MODES}


def same_nonfinite(out, exp, what):
    o, e = out.float().cpu(), exp.float().cpu()
    assert o.shape == e.shape and out.dtype == exp.dtype, f"{what}: {tuple(o.shape)} {out.dtype} vs {tuple(e.shape)} {exp.dtype}"
    for fn in (torch.isnan, torch.isposinf, torch.isneginf):
        a, b = fn(o), fn(e)
        if not torch.equal(a, b):
            bad = (a != b).nonzero()[0].tolist()
            raise AssertionError(f"{what}: {fn.__name__} at {int(a.sum())} places, expected {int(b.sum())}; first difference at {bad}: "
                                 f"got {float(o[tuple(bad)])}, expected {float(e[tuple(bad)])}")
    return torch.isfinite(e)


def close_to_reference(out, exp, mode, stride, what):
    """NaN, +Inf and -Inf at identical positions; finite values by tests/_golden.pool_close_enough's bars (max pooling and stride 1
    exact, bf16 one ulp, fp32 2e-6 absolute on unit-variance inputs -- made relative to the scale of the scaled clips, exactly: the
    scalings are powers of two)."""
    from tests._golden import pool_close_enough
    fin = same_nonfinite(out, exp, what)
    o = torch.where(fin, out.cpu().float(), torch.zeros(())).to(out.dtype)
    e = torch.where(fin, exp.cpu().float(), torch.zeros(())).to(exp.dtype)
    scale = 1.0
    m = float(e.float().abs().max())
    if m > 2.0 ** 40:
        scale = 2.0 ** -62
    elif 0 < m < 2.0 ** -40:
        scale = 2.0 ** 70
    if scale != 1.0:
        o, e = (o.float() * scale).to(out.dtype), (e.float() * scale).to(exp.dtype)
    assert pool_close_enough(o, e, dict(mode=mode, stride=stride)), f"{what}: finite values differ from the reference"


def bits_equal(a, b):
    """bit equality (NaN payloads included are NOT compared: NaN positions equal, everything else bit-equal)"""
    a, b = a.cpu(), b.cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = torch.isnan(a.float()), torch.isnan(b.float())
    view = torch.int32 if a.element_size() == 4 else torch.int16
    return torch.equal(na, nb) and torch.equal(a.contiguous().view(view)[~na], b.contiguous().view(view)[~nb])
