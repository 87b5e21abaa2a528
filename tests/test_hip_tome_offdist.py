"""GPU parity of the ToMe kernels away from synth-v1 (tests/_tome_offdist.py):

1. every family of tests/golden/tomeod_*.npz (the reference's own outputs on NaN / Inf / all-zero tokens, constant and duplicated
   clips, norms that underflow and overflow, float16 merge sums past 65 504, a NaN in one head) through get_tome_features: same ids,
   same NaN / Inf pattern, finite values within the project's bounds, no id or row slack;
2. every match kernel on a poisoned b-row (inside a full tile, inside the last partial tile, at j = 0, at j = nb - 1) and a poisoned
   a-row, against a dense product with torch.max semantics;
3. the ranking with some, and with only, NaN keys against a stable descending argsort;
4. the per-snippet path with one poisoned b-token in one snippet;
5. the 16-bit dispatch branches no other test reaches (scalar normalise, 4- and 1-channel merge, a misaligned base pointer).
"""
import pytest
import torch

from tests import _tome_offdist as D

pytestmark = pytest.mark.gpu

TOME_DEFAULT_SPLIT = 2
CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _step(x, r):
    """One sttm_tome_step on tokens x [n, C] (device): (x_out, idx_out, node_max, node_idx)."""
    from sttm_amd import _lib
    lib = _lib.load()
    dev = x.device
    n, C = x.shape
    na = (n + 1) // 2
    nbytes = lib.sttm_tome_workspace_bytes(n, C, 1)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    xo = torch.empty((n - r, C), dtype=x.dtype, device=dev)
    so = torch.empty(n - r, device=dev)
    io = torch.empty(n - r, dtype=torch.int64, device=dev)
    nmax = torch.empty(na, device=dev)
    nidx = torch.empty(na, dtype=torch.int32, device=dev)
    rc = lib.sttm_tome_step(x.data_ptr(), None, None, n, C, 1, r, CODE[x.dtype], ws.data_ptr(), nbytes, xo.data_ptr(), so.data_ptr(),
                            io.data_ptr(), nmax.data_ptr(), nidx.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.raise_for(rc)
    torch.cuda.synchronize()
    return xo, io, nmax, nidx


# ----------------------------------------------------------------------------------------------
# 1. the reference's outputs on every family
# ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fid", D.fixture_ids())
def test_fixture_parity(fid):
    """Default dispatch at these sizes: k_tome_normalize_split<4> + k_tome_match_split<32, 2, 2, 3> (fp32), k_tome_normalize16<T, 8> +
    k_tome_match16<T> (16-bit), k_tome_rank, k_tome_merge<T, 4 / 8>; nan_head4 takes the scalar normalise kernels (n_head > 1).  A
    poisoned b-row or a constant clip sends every source to ONE destination: the merge kernel's list sort and sum for more than 64 sources."""
    from sttm_amd import get_tome_features
    c = D.load_fixture(fid)
    x = c["x"].to(_dev())
    for ratio, (efeat, eidx) in c["out"].items():
        feat, idx = get_tome_features(x, ratio, "video", c["meta"]["n_head"])
        D.assert_matches_fixture(feat, idx, efeat, eidx, ratio, f"{fid} r={ratio}")


# ----------------------------------------------------------------------------------------------
# 2. every match kernel on poisoned rows
# ----------------------------------------------------------------------------------------------

# na -> (a b-row inside a full tile of the kernels that have one at this size, a b-row inside the last partial tile)
PLACES = {100: (50, 90), 300: (130, 280), 700: (300, 690)}


def _poison(tok, row, kind):
    if kind == "zero":
        tok[row] = 0
    elif kind == "tiny":                      # norm underflow: a +-Inf unit row without a NaN
        tok[row] = (tok[row].float() * 1e-30).to(tok.dtype)
    else:
        tok[row, 7] = float("nan") if kind == "nan" else float("inf")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_every_match_kernel_on_poisoned_rows(dtype):
    """tome_split 0 = k_tome_match (fp32 MFMA), 3 / 5 = k_tome_match_split (4 / 3 terms; 16-bit: k_tome_match16), 4 / 6 = k_tome_match_glds
    with eight waves, 7 = its four-wave AGPR form; tome_flat 0 / 2 = per-a-tile and flat work split of the 256-tile kernels.  na = 100: below
    one tile; 300: one full 256-tile and a partial one (two full 128-tiles and a partial one); 700: ragged.  A poisoned b-row makes every
    clean a-row (NaN, that row); a poisoned a-row is (NaN, 0) and leaves the others alone.  Poisoned: a NaN or Inf element, an all-zero
    token, or a token scaled by 1e-30 ("tiny": its norm underflows, its unit row is +-Inf and its 64 products have both signs)."""
    from sttm_amd import _lib
    dev = _dev()
    g = torch.Generator().manual_seed(31)
    C = 64
    worst_err, worst_agree = 0.0, 1.0
    modes = [(m, 1) for m in ((0, 3, 4, 5, 6, 7) if dtype == torch.float32 else (3, 4, 7))] + [(4, 0), (4, 2), (7, 0), (7, 2)]
    try:
        for na, (j_full, j_part) in PLACES.items():
            n = 2 * na
            base = torch.randn(n, C, generator=g).to(dtype)
            cases = [("b", j_full, "nan"), ("b", j_part, "zero"), ("b", 0, "inf"), ("b", na - 1, "nan"), ("b", j_full + 1, "tiny"),
                     ("a", na // 3, "zero"), ("a", na - 1, "inf"), ("a", 1, "tiny")]
            for side, row, kind in cases:
                tok = base.clone()
                _poison(tok, 2 * row + (side == "b"), kind)
                ref_max, ref_idx = D.dense_match_reference(tok, dtype)
                nan_ref = torch.isnan(ref_max)
                assert int(nan_ref.sum()) == (na if side == "b" else 1)
                assert bool((ref_idx[nan_ref] == (row if side == "b" else 0)).all())
                x = tok.to(dev)
                for mode, flat in modes:
                    _lib.configure(tome_split=mode, tome_flat=flat)
                    _, _, nmax, nidx = _step(x, na)
                    nmax, nidx = nmax.cpu(), nidx.long().cpu()
                    what = f"{dtype} na={na} {side}-row {row} {kind} tome_split={mode} tome_flat={flat}"
                    nan = torch.isnan(nmax)
                    assert torch.equal(nan, nan_ref), f"{what}: {int(nan.sum())} NaN rows, expected {int(nan_ref.sum())}"
                    bad = (nidx[nan] != ref_idx[nan]).nonzero().flatten()
                    assert bad.numel() == 0, f"{what}: {bad.numel()} NaN rows with another node_idx, first got {int(nidx[nan][bad[0]])}, expected {int(ref_idx[nan][bad[0]])}"
                    fin = ~nan
                    if bool(fin.any()):
                        agree = (nidx[fin] == ref_idx[fin]).float().mean().item()
                        worst_agree = min(worst_agree, agree)
                        if dtype == torch.float32:            # the bounds of test_tome_match_kernel_variants
                            err = float((nmax[fin].double() - ref_max[fin]).abs().max())
                            worst_err = max(worst_err, err)
                            assert err < 2e-6 and agree > 0.999, f"{what}: finite rows: max |best - float64| {err:.3e}, argmax agreement {agree:.5f}"
                        else:
                            # both sides round an fp32-accumulated sum of the same 64 products to the dtype: the sums differ by the
                            # accumulation order (~1e-6), so a rounded score differs by at most one ulp of a value below 1 (2^-8 bf16,
                            # 2^-11 fp16); the argmax share is the one of test_tome_16bit_match_scores_against_dense_reference
                            err = float((nmax[fin] - ref_max[fin]).abs().max())
                            worst_err = max(worst_err, err)
                            ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
                            assert err <= ulp and agree > 0.97, f"{what}: finite rows: max |best - reference| {err:.3e}, argmax agreement {agree:.4f}"
        print(f"{dtype}: finite rows over all kernels and placements: max |best - reference| {worst_err:.3e}, lowest argmax agreement {worst_agree:.5f}")
    finally:
        _lib.configure(tome_split=TOME_DEFAULT_SPLIT, tome_flat=1)


# ----------------------------------------------------------------------------------------------
# 3. ranking with NaN keys
# ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("poisoned", ["some_a_rows", "one_b_row"])
def test_ranking_with_nan_keys(dtype, poisoned):
    """k_tome_rank with several NaN row maxima (poisoned a-rows, in both 256-key blocks) and with nothing but NaN row maxima (one
    poisoned b-row): the unmerged even tokens come out in the order of torch's STABLE descending argsort of the kernel's own best
    scores (NaN first, ties to the smaller index)."""
    from sttm_amd.synth import synth_video
    x = synth_video(3, 64, 14, 14, seed=41, dtype=dtype).permute(0, 2, 3, 1).reshape(-1, 64).clone()
    n = x.shape[0]
    na, r = n // 2, 200
    if poisoned == "some_a_rows":
        for i in (3, 77, 255, 256, 293):
            x[2 * i] = 0
    else:
        x[2 * 101 + 1, 9] = float("nan")
    _, io, nmax, nidx = _step(x.to(_dev()), r)
    nmax = nmax.cpu()
    n_nan = int(torch.isnan(nmax).sum())
    assert n_nan == (5 if poisoned == "some_a_rows" else na)
    order = torch.argsort(nmax, descending=True, stable=True)
    assert bool(torch.isnan(nmax[order[:n_nan]]).all())
    assert torch.equal(io.cpu()[:na - r], 2 * order[r:]), "unmerged even tokens are not in stable descending order"
    assert torch.equal(io.cpu()[na - r:], 2 * torch.arange(n // 2) + 1)
    if poisoned == "one_b_row":
        assert bool((nidx.cpu() == 101).all()) and torch.equal(order, torch.arange(na))


# ----------------------------------------------------------------------------------------------
# 4. the per-snippet path
# ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("S", [1, 2])
def test_snippet_with_one_poisoned_b_token(S, dtype):
    """k_tsn_normalize / k_tsn_match / k_tsn_rank / k_tsn_merge on a T = 4 clip with a NaN element in one b-token of frame 2: the
    snippet that holds it equals the reference's per-video result on that sub-video (every a-token merged into the poisoned b-token;
    ratio 0.75 runs a second iteration, in which the poisoned row 20 is an a-token), every other snippet its clean result.  Segments of
    196 and 392 tokens merge every a-token at both ratios, so no cut runs through the tied NaN keys (tests/_tome_offdist.py)."""
    from oracle import sttm_oracle as O
    from sttm_amd import get_tome_features_snippet
    from sttm_amd.synth import synth_video
    T, C, H, W = 4, 32, 14, 14
    x = synth_video(T, C, H, W, seed=43, dtype=dtype)
    x.permute(0, 2, 3, 1)[2].reshape(-1, C)[41, 5] = float("nan")
    xd = x.to(_dev())
    for ratio in (0.5, 0.75):
        feat, idx = get_tome_features_snippet(xd, ratio, S)
        feat, idx = feat.cpu(), idx.cpu()
        a = 0
        for g in range(T // S):
            sub = x[g * S:(g + 1) * S]
            ok, why = D.well_determined(sub, ratio)
            assert ok, why
            ef, ei = O.get_tome_features(sub, ratio, "video", 1)
            b = a + ef.shape[0]
            poisoned = g == 2 // S
            assert bool(torch.isnan(ef.float()).any()) == poisoned
            D.assert_matches_fixture(feat[a:b], idx[a:b] - g * S * H * W, ef, ei, ratio, f"{dtype} S={S} r={ratio} snippet {g}")
            a = b
        assert a == feat.shape[0]


# ----------------------------------------------------------------------------------------------
# 5. 16-bit dispatch branches without a test elsewhere
# ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("C", [100, 250, 4104])
def test_16bit_scalar_normalise_and_narrow_merge(dtype, C):
    """C = 100:  k_tome_normalize16<T, 1> (C % 8 != 0) and k_tome_merge<T, 4>.
    C = 250:  k_tome_normalize16<T, 1> and k_tome_merge<T, 1> (C % 4 != 0).
    C = 4104: k_tome_normalize16<T, 1> (above the 4096-channel cap of the vector form) and k_tome_merge<T, 8>.
    Against the oracle under the bound of the other 16-bit oracle cases."""
    from oracle import sttm_oracle as O
    from sttm_amd import get_tome_features
    from sttm_amd.synth import synth_video
    from tests.test_hip_parity import _assert_tome16, _tome16_agreement
    x = synth_video(2, C, 14, 14, seed=900 + C, dtype=dtype)
    ef, ei = O.get_tome_features(x, 0.7, "video", 1)
    f, i = get_tome_features(x.to(_dev()), 0.7, "video", 1)
    assert f.dtype == dtype and f.shape == ef.shape
    what = f"{dtype} C={C}"
    ida, fa = _tome16_agreement(f, i, ef, ei, what)
    _assert_tome16(ida, fa, ei.numel(), what)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_16bit_step_on_a_misaligned_base_pointer(dtype):
    """x starts 2 bytes off a 16-byte boundary (a slice of a larger buffer), C = 64: k_tome_normalize16<T, 1> and k_tome_merge<T, 1>
    although C % 8 == 0.  One step at r = n // 2 against the oracle."""
    from oracle import sttm_oracle as O
    from sttm_amd.synth import synth_video
    from tests.test_hip_parity import _assert_tome16, _tome16_agreement
    x4 = synth_video(2, 64, 14, 14, seed=77, dtype=dtype)
    tok = x4.permute(0, 2, 3, 1).reshape(-1, 64)
    n, C = tok.shape
    buf = torch.empty(n * C + 8, dtype=dtype, device=_dev())
    assert buf.data_ptr() % 16 == 0
    x = buf[1:1 + n * C].view(n, C)
    x.copy_(tok)
    assert x.data_ptr() % 16 == 2 and x.is_contiguous()
    xo, io, _, _ = _step(x, n // 2)
    ef, ei = O.get_tome_features(x4, 0.5, "video", 1)
    assert torch.equal(io.cpu(), ei)
    ida, fa = _tome16_agreement(xo, io, ef, ei, f"{dtype} misaligned")
    _assert_tome16(ida, fa, ei.numel(), f"{dtype} misaligned")
