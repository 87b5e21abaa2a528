"""Off-distribution inputs for the ToMe baseline: NaN / Inf / all-zero tokens, exact ties (duplicated and constant clips), norms that
underflow or overflow, float16 merge sums past 65 504, a NaN in one head of a head-mean metric.  Shared by
tests/test_tome_offdist_cpu.py, tests/test_hip_tome_offdist.py and tests/golden/make_golden_tome_offdist.py.  Everything here runs on the
CPU; nothing imports the device library.

What the reference does with a poisoned token (tome_token_merger.py:32-41): `metric / metric.norm()` turns a token with a NaN, an Inf
(inf / inf) or nothing but zeros (0 / 0) into a unit row that holds a NaN, and a token whose sum of squares underflows into a unit row
of +-Inf, so every score against it is NaN (a NaN product, or infinities of both signs in one sum).  `scores.max(-1)`
propagates NaN and returns the FIRST NaN's index, `argsort(descending=True)` puts NaN first -- tied keys in an order of the sort's own
once there are more than 16.  A poisoned b-token (odd flat index) therefore makes node_max NaN for EVERY a-row, node_idx that b-row for
every a-row whose own unit row is clean, and r a-tokens are merged into it (all of them in the committed shapes); a poisoned a-token
(even flat index) has (NaN, 0) itself and is ranked first.

A family is a plain function of (T, C, H, W, seed, dtype) that starts from synth_video and edits it in THWC order; the edited token is
named by its flat index t * H * W + y * W + x, whose parity decides the side (a = even, b = odd).
"""
import json
import math
import os

import numpy as np
import torch

from oracle import sttm_oracle as O
from sttm_amd.synth import synth_video
from tests._golden import GOLDEN_DIR, _t
from tests._offdist import DTYPES, FP32_TOL, SHORT, bits_equal_nan_aware

NAN, INF = float("nan"), float("inf")


def _family(edit):
    def build(T, C, H, W, seed, dtype):
        x = synth_video(T, C, H, W, seed=seed, dtype=dtype)
        m = x.permute(0, 2, 3, 1)                 # the [T, H, W, C] memory
        assert m.is_contiguous()
        edit(m.reshape(T * H * W, C), m)          # (tokens by flat index -- a view --, the frames)
        return x
    return build


def _last_b(n):
    return n - 1 if n % 2 == 0 else n - 2


def _set_tokens(value, *tokens, ch=None):
    def edit(tok, _m):
        for i in tokens:
            i = i(tok.shape[0]) if callable(i) else i
            if ch is None:
                tok[i] = value
            else:
                tok[i, ch] = value
    return edit


def _scale(s):
    def edit(tok, _m):
        tok.copy_((tok.float() * s).to(tok.dtype))
    return edit


def _tiny_token(i):
    def edit(tok, _m):
        tok[i] = (tok[i].float() * 1e-30).to(tok.dtype)          # the sum of squares underflows: norm 0, unit row +-Inf, no NaN in it
    return edit


def _zero_frame(_tok, m):
    m[1] = 0


def _zero_video(tok, _m):
    tok.zero_()


def _const_video(tok, _m):
    tok[:] = tok[0].clone()


def _dup_frames(_tok, m):
    m[1:] = m[0].clone()          # 7 x 7: a frame has 49 tokens, so a token's copy in the next frame has the other parity


def _f16_merge_overflow(tok, _m):
    tok[:] = (tok[0].float() * 300.0).to(tok.dtype)        # |x| up to a few hundred, every token the same


A_TOK, B_TOK = 40, 41            # one a-token and one b-token in the middle of the first frame (b-row j = 20)
# name -> (builder, (T, C, H, W), n_head, dtypes, ratios).  Every ratio list holds 0.5 (one iteration, r = n // 2) and one ratio that
# needs at least two iterations.  The reference's `argsort(descending=True)` is NOT stable beyond 16 keys (ATen's CPU sort: tied keys --
# all the NaN row maxima a poisoned b-token produces, all the equal ones of a constant clip -- come out in an order of the sort's own,
# see `well_determined`), so wherever an iteration ranks tied keys the shapes and ratios are chosen such that it merges EVERY a-token
# (n even, r = n // 2: 196 -> 98 -> 49 at ratio 0.75) and no cut runs through the tie.
BOTH = ("float32", "bfloat16")
STD, RATIOS = (4, 32, 7, 7), (0.5, 0.75)
FAMILIES = {
    "zero_a_token": (_family(_set_tokens(0.0, A_TOK)), STD, 1, BOTH, RATIOS),
    # n odd: the cut leaves one a-token, and the zero token's NaN row ranks first in front of it (the merged b-token 1 stays finite)
    "zero_a_token_cut": (_family(_set_tokens(0.0, A_TOK)), (3, 32, 7, 7), 1, BOTH, (0.5, 0.7)),
    "zero_b_token": (_family(_set_tokens(0.0, B_TOK)), STD, 1, BOTH, RATIOS),
    "nan_elem_a": (_family(_set_tokens(NAN, A_TOK, ch=5)), STD, 1, BOTH, RATIOS),
    "nan_elem_b": (_family(_set_tokens(NAN, B_TOK, ch=5)), STD, 1, BOTH, RATIOS),
    "inf_elem_a": (_family(_set_tokens(INF, A_TOK, ch=5)), STD, 1, BOTH, RATIOS),
    "inf_elem_b": (_family(_set_tokens(INF, B_TOK, ch=5)), STD, 1, BOTH, RATIOS),
    # one token whose norm underflows among clean ones: its scores sum infinities of both signs (32 products: all of one sign in
    # 2^-31 of the rows), so they are NaN like a poisoned token's
    "tiny_a_token": (_family(_tiny_token(A_TOK)), STD, 1, BOTH, RATIOS),
    "tiny_b_token": (_family(_tiny_token(B_TOK)), STD, 1, BOTH, RATIOS),
    "nan_two_b": (_family(_set_tokens(NAN, 91, B_TOK, ch=5)), STD, 1, BOTH, RATIOS),       # j = 45 and j = 20: 20 wins
    "nan_b_first": (_family(_set_tokens(NAN, 1, ch=5)), STD, 1, BOTH, RATIOS),              # j = 0
    "nan_b_last": (_family(_set_tokens(NAN, _last_b, ch=5)), STD, 1, BOTH, RATIOS),         # j = nb - 1 (odd: a b-token again in iteration 2)
    "zero_frame": (_family(_zero_frame), STD, 1, BOTH, RATIOS),                             # zero a-rows (NaN, 0), clean a-rows (NaN, 24)
    "zero_video": (_family(_zero_video), STD, 1, BOTH, RATIOS),
    "const_video": (_family(_const_video), STD, 1, BOTH, RATIOS),
    "dup_frames": (_family(_dup_frames), (2, 32, 7, 7), 1, BOTH, (0.5, 0.7)),
    "scale_1e-30": (_family(_scale(1e-30)), STD, 1, BOTH, RATIOS),        # sum of squares underflows: norm 0, unit rows +-inf
    "scale_1e+20": (_family(_scale(1e20)), STD, 1, BOTH, RATIOS),         # sum of squares overflows: norm inf, unit rows 0
    "f16_scale_inf": (_family(_scale(1e5)), STD, 1, ("float16",), RATIOS),      # elements past 65 504 become Inf
    "f16_merge_overflow": (_family(_f16_merge_overflow), (8, 32, 7, 7), 1, ("float16",), (0.5, 0.875)),      # 392 -> 196 -> 98 -> 49
    "nan_head4": (_family(_set_tokens(NAN, B_TOK, ch=3)), (4, 64, 7, 7), 4, BOTH, RATIOS),    # head 0 only: the head mean spreads it
    "nan_elem_b_14": (_family(_set_tokens(NAN, 301, ch=9)), (2, 32, 14, 14), 1, BOTH, RATIOS),   # two 128-row a-tiles, j = 150
}
DEFAULT_SEED = 5
# (family, dtype) -> seed, where the default seed's clip was rejected by `well_determined` (profiles/tome_offdist.md lists why)
SEEDS = {}


def seed_of(name, dname):
    return SEEDS.get((name, dname), DEFAULT_SEED)


def fixture_ids():
    return [f"tomeod_{name}_{SHORT[d]}" for name, (_, _, _, dts, _) in FAMILIES.items() for d in dts]


def build(name, dname, seed=None):
    fn, shape, _, _, _ = FAMILIES[name]
    return fn(*shape, seed_of(name, dname) if seed is None else seed, DTYPES[dname])


def ratio_key(ratio):
    return f"r{int(round(ratio * 100)):03d}"


def load_fixture(fid):
    """tests/golden/tomeod_*.npz -> dict(meta, x, out={ratio: (feat, idx)}).  One file per family and dtype: the input once, the
    reference's outputs for every ratio of the family."""
    z = np.load(os.path.join(GOLDEN_DIR, fid + ".npz"))
    meta = json.loads(str(z["meta"]))
    d = meta["dtype"]
    x = _t(z["x_thwc"], d).permute(0, 3, 1, 2)
    out = {r: (_t(z["feat_" + ratio_key(r)], d), torch.from_numpy(z["idx_" + ratio_key(r)])) for r in meta["ratios"]}
    return dict(meta=meta, x=x, out=out)


# ----------------------------------------------------------------------------------------------
# the oracle's loop with its decisions recorded, in the reference's arithmetic or with float64 scores
# ----------------------------------------------------------------------------------------------

def tome_trace(x_tchw, ratio, n_head=1, scores64=False):
    """O.get_tome_features(x, ratio, "video", n_head) with every iteration's (node_max, node_idx) recorded.  scores64: the score
    product of the (reference-dtype) unit rows in float64 -- rounded to the input dtype for 16-bit inputs, whose score tensor has that
    dtype -- instead of the dtype's own matmul.  Returns (feat, idx, [(node_max, node_idx, the cut separates two tied keys), ...])."""
    rec = []
    orig = O.tome_match

    def match(metric, r):
        m = metric / metric.norm(dim=-1, keepdim=True)
        a, b = m[0::2], m[1::2]
        if scores64:
            s = a.double() @ b.double().transpose(-1, -2)
            if metric.dtype != torch.float32:
                s = s.to(metric.dtype)
        else:
            s = a @ b.transpose(-1, -2)
        best, arg = s.max(dim=-1)
        order = best.argsort(dim=-1, descending=True)
        k = best.float()[order]
        tied = bool(r < k.numel() and (k[r - 1] == k[r] or (torch.isnan(k[r - 1]) and torch.isnan(k[r]))))
        rec.append((best, arg, tied))
        return order[r:], order[:r], arg[order[:r]]

    O.tome_match = match
    try:
        feat, idx = O.get_tome_features(x_tchw, ratio, "video", n_head)
    finally:
        O.tome_match = orig
    return feat, idx, rec


def well_determined(x_tchw, ratio, n_head=1):
    """A clip may ask for exact ids only if the reference alone is well determined on it: the same loop with float64 scores takes the
    same node_idx in every iteration (NaN rows compared as a mask) and keeps the same ids, and no top-r cut separates two tied row
    maxima (equal, or both NaN): `argsort(descending=True)` is not stable -- ATen's CPU sort returns tied keys in index order only up to
    16 of them -- so which of the tied a-tokens are merged is the sort's business there, not the reference's definition (the device
    ranks ties by the smaller index, tome.hip).  Returns (ok, reason)."""
    _, i32, r32 = tome_trace(x_tchw, ratio, n_head)
    _, i64, r64 = tome_trace(x_tchw, ratio, n_head, scores64=True)
    if len(r32) != len(r64):
        return False, "iteration counts differ"
    for k, ((b32, a32, tied), (b64, a64, _)) in enumerate(zip(r32, r64)):
        if tied:
            return False, f"iteration {k}: the top-r cut separates tied row maxima (unstable argsort)"
        if b32.shape != b64.shape:
            return False, f"iteration {k}: shapes differ"
        if not torch.equal(torch.isnan(b32.float()), torch.isnan(b64.float())):
            return False, f"iteration {k}: NaN rows differ"
        if not torch.equal(a32, a64):
            bad = (a32 != a64).nonzero().flatten()
            return False, f"iteration {k}: node_idx of {bad.numel()} rows differs with float64 scores (an argmax near-tie), first row {int(bad[0])}"
    if not torch.equal(i32, i64):
        return False, "kept ids differ with float64 scores (a near-tie at the top-r cut)"
    return True, ""


def tome_with_device_rules(x_tchw, ratio, n_head=1):
    """The loop restated with the rules the kernels add where the reference leaves a choice: row maxima ranked by a STABLE descending
    sort (ties to the smaller index), a destination's sources added in rank order, 16-bit sums accumulated in fp32 and rounded once
    (tome.hip, k_tome_merge).  Scores, maxima and every other rounding are the reference's.  CPU only, slow, for the fixture shapes."""
    T, C, H, W = x_tchw.shape
    x = x_tchw.permute(0, 2, 3, 1).reshape(T * H * W, C)
    dt = x.dtype
    n = x.shape[0]
    target = math.ceil(n * (1 - ratio))
    idx = torch.arange(n)
    size = torch.ones(n, 1, dtype=dt)
    first = True
    while first or x.shape[0] > target:
        first = False
        n = x.shape[0]
        r = min(n - target, n // 2)
        metric = x.reshape(n, n_head, C // n_head).mean(1)
        m = metric / metric.norm(dim=-1, keepdim=True)
        best, arg = (m[0::2] @ m[1::2].transpose(-1, -2)).max(dim=-1)
        order = best.argsort(dim=-1, descending=True, stable=True)
        src, unm = order[:r], order[r:]
        dst = arg[src]

        def merge(v):
            va, acc = v[0::2], v[1::2].float().clone()
            for k in range(r):
                acc[dst[k]] += va[src[k]].float()
            return torch.cat([va[unm], acc.to(dt)], dim=0)

        xs = merge(x * size)
        size = merge(size)
        x = xs / size
        idx = torch.cat([idx[0::2][unm], idx[1::2]])
    return x, idx


# ----------------------------------------------------------------------------------------------
# comparisons
# ----------------------------------------------------------------------------------------------

def _as_map(feat, idx):
    order = torch.argsort(idx)
    return idx[order], feat[order]


def assert_matches_fixture(feat, idx, efeat, eidx, ratio, what):
    """Device output against the reference's: ids as sets (positionally at ratio 0.5), NaN / +Inf / -Inf masks of the features equal,
    finite values within FP32_TOL (fp32) or 2 ulps of the input dtype (16-bit: the rule of _tome16_agreement), relative to
    max(1, |expected|).  No id or row slack: the families hold no near-tie (well_determined)."""
    feat, idx = feat.cpu(), idx.cpu()
    assert feat.dtype == efeat.dtype and idx.dtype == torch.int64 and feat.shape == efeat.shape, f"{what}: shapes / dtypes"
    gi, gf = _as_map(feat, idx)
    xi, xf = _as_map(efeat, eidx)
    if not torch.equal(gi, xi):
        only_g, only_x = sorted(set(gi.tolist()) - set(xi.tolist())), sorted(set(xi.tolist()) - set(gi.tolist()))
        raise AssertionError(f"{what}: kept ids differ: only here {only_g[:8]}, only in the reference {only_x[:8]} ({len(only_x)} of {len(xi)})")
    if ratio == 0.5:
        assert torch.equal(idx, eidx), f"{what}: ids not positionally equal at ratio 0.5"
    g, e = gf.float(), xf.float()
    for name, fn in (("NaN", torch.isnan), ("+Inf", torch.isposinf), ("-Inf", torch.isneginf)):
        a, b = fn(g), fn(e)
        if not torch.equal(a, b):
            bad = (a != b).nonzero()
            raise AssertionError(f"{what}: {name} positions differ ({int(a.sum())} vs {int(b.sum())} expected), first at token id "
                                 f"{int(xi[bad[0][0]])} channel {int(bad[0][1])}: got {float(g[tuple(bad[0])])}, expected {float(e[tuple(bad[0])])}")
    tol = FP32_TOL if feat.dtype == torch.float32 else (2.0 ** -6 if feat.dtype == torch.bfloat16 else 2.0 ** -9)
    fin = torch.isfinite(e)
    err = torch.where(fin, (g - e).abs() / e.abs().clamp_min(1.0), torch.zeros_like(e))
    worst = float(err.max()) if err.numel() else 0.0
    print(f"{what}: {len(xi)} ids equal, NaN {int(torch.isnan(e).sum())} Inf {int(torch.isinf(e).sum())}, max finite rel err {worst:.3e} (tol {tol:.1e})")
    if worst > tol:
        rows = (err > tol).any(dim=1).nonzero().flatten()
        raise AssertionError(f"{what}: {rows.numel()} rows beyond {tol:.1e} (max {worst:.3e}), token ids {xi[rows][:8].tolist()}")


def dense_match_reference(x, dtype):
    """node_max / node_idx of one step on tokens x [n, C] with torch.max semantics (NaN propagates, first NaN / first maximum): the
    product of the unit rows in float64 for fp32 inputs, fp32-accumulated then rounded to the dtype for 16-bit inputs."""
    m = x / x.norm(dim=-1, keepdim=True)
    if dtype == torch.float32:
        s = m[0::2].double() @ m[1::2].double().T
    else:
        s = (m[0::2].float() @ m[1::2].float().T).to(dtype).float()
    return s.max(dim=-1)


def kept_count(n, ratio):
    return math.ceil(n * (1 - ratio))


__all__ = ["FAMILIES", "fixture_ids", "build", "load_fixture", "tome_trace", "well_determined", "assert_matches_fixture",
           "dense_match_reference", "tome_with_device_rules", "bits_equal_nan_aware", "kept_count", "ratio_key", "seed_of"]
