"""GPU tests of the two DyCoke kernel files off the distribution their own suites use (inputs and case tables: tests/_dycoke_offdist.py,
where every parameter is written next to the kernel instantiation or loop trip it reaches).

  stage 1 (csrc/dycoke.hip)         every width class of launch_dycoke against the oracle, the P and k edges of k_dycoke_select, clips
                                    with non-finite or degenerate tokens against the reference-made dycod_* vectors
  stage 2 (csrc/dycoke_decode.hip)  group sizes past one sweep of kDecGmax heads, a peaked logit family with an attention sink,
                                    non-finite cache rows, awkward layouts, keep lists with skipped entries

The Gaussian stage-2 cases keep the allowances of tests/test_hip_dycoke_decode.py unchanged.  The peaked family has its own, measured
the same way on its own cases (profiles/dycoke_offdist.md records the values)."""
import functools

import pytest
import torch

from tests import _dycoke_decode_ref as R
from tests import _dycoke_offdist as DO
from tests.test_hip_dycoke import _compare
from tests.test_hip_dycoke_decode import _attn_err, _rel, attn_allowance, make_qkv, score_allowance

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ---- stage 1: width classes ---------------------------------------------------------------------------------------------------------
def _against_oracle(x, T, prune, x_dev=None):
    from oracle import dycoke_oracle as D
    from sttm_amd.dycoke_merger import dycoke_ttm
    P = x.shape[0] // T
    ef, ei, sims = D.dycoke_ttm(x, T, prune, return_sims=True)
    out, oi = dycoke_ttm(x.to(DEV) if x_dev is None else x_dev, T, prune)
    out, oi = out.cpu(), oi.cpu()
    exact = _compare(out, oi, ef, ei, sims, P, int((1 - prune) * P))
    assert int(oi.min()) >= 0 and int(oi.max()) < x.shape[0]
    assert torch.equal(out, x[oi])                                             # rows are exact copies of the chosen tokens
    return exact, oi


@pytest.mark.parametrize("C,family,seed", DO.FP32_WIDTHS, ids=lambda v: str(v))
def test_stage1_fp32_width_classes(C, family, seed):
    x = DO.stage1_input(family, DO.WIDTH_T, C, DO.WIDTH_SIDE, DO.WIDTH_SIDE, seed)
    exact, _ = _against_oracle(x, DO.WIDTH_T, DO.WIDTH_PRUNE)
    print(f"fp32 C={C} ({family}): ids {'equal' if exact else 'equal up to similarities closer than 1e-6'}")


def test_stage1_fp32_input_off_the_16_byte_boundary():
    """C = 64 rows whose storage starts 4 bytes past a 16-byte boundary: `.contiguous()` has nothing to do, so dycoke_ttm hands the
    kernel that pointer and launch_dycoke must take k_dycoke_sim<0> / k_dycoke_gather<0> (no 16-byte loads)."""
    T, C, side = DO.WIDTH_T, 64, DO.WIDTH_SIDE
    x = DO.stage1_input("iid", T, C, side, side, 10)
    buf = torch.zeros(x.numel() + 1, device=DEV)
    xd = buf[1:].view(x.shape)
    xd.copy_(x)
    assert xd.is_contiguous() and xd.data_ptr() % 16 == 4 and xd.contiguous().data_ptr() == xd.data_ptr()
    _against_oracle(x, T, DO.WIDTH_PRUNE, x_dev=xd)


@pytest.mark.parametrize("C,family,seed,dname", DO.LOWP_CASES, ids=lambda v: str(v))
def test_stage1_16bit_width_classes(C, family, seed, dname):
    from sttm_amd.dycoke_merger import dycoke_ttm
    x, ref = DO.lowp_reference(C, family, seed, dname)
    out, oi = dycoke_ttm(x.to(DEV), DO.WIDTH_T, DO.WIDTH_PRUNE)
    differ = ref.check(out.cpu(), oi.cpu(), x)
    print(f"{dname} C={C}: {differ} of {ref.kept} kept tokens differ from the stable sort ({ref.near} within 2 ulps of a cut)")


@pytest.mark.parametrize("T,C", DO.ODD_T_CASES)
def test_stage1_odd_frame_counts_through_the_wide_gather(T, C):
    x = DO.stage1_input("synth", T, C, DO.WIDTH_SIDE, DO.WIDTH_SIDE, 30 + T)
    _, oi = _against_oracle(x, T, DO.WIDTH_PRUNE)
    P = DO.WIDTH_SIDE ** 2
    assert oi[-P:].tolist() == list(range((T - 1) * P, T * P))                # the odd last frame is whole


@pytest.mark.parametrize("H,W", DO.P_EDGES, ids=lambda v: str(v))
def test_stage1_tokens_per_frame_and_k_edges(H, W):
    T, C, P = 5, 16, H * W
    x = DO.stage1_input("iid", T, C, H, W, 40)
    # prune_ratio 0: k = P, every frame complete, pruned frames in ascending-similarity order; then the ratio that gives k = 1
    # (for P = 1 the first pass already has k = 1, and the ratio of the second would be negative: one pass)
    for prune in ((0.0,) if P == 1 else (0.0, 1.0 - 1.5 / P)):
        k = int((1 - prune) * P)
        assert 0.0 <= prune < 1.0 and k == (P if prune == 0.0 else 1)
        _, oi = _against_oracle(x, T, prune)
        assert oi.numel() == 2 * P + 3 * k                                     # frames 0 and 4 whole; 1, 3 (pass 1) and 2 (pass 2) pruned
        if k == P:
            assert sorted(oi.tolist()) == list(range(T * P))


def test_stage1_more_than_2048_tokens_per_frame_raises():
    from sttm_amd.dycoke_merger import dycoke_ttm
    H, W = DO.P_TOO_MANY
    x = torch.zeros(5 * H * W, 16, device=DEV)
    with pytest.raises(NotImplementedError, match="2048 tokens per frame"):
        dycoke_ttm(x, 5, 0.5)


# ---- stage 1: degenerate clips --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", DO.degenerate_ids())
def test_stage1_degenerate_clips(fid):
    """Against the reference-made vectors.  The clips of DO.DEG_NONFINITE hold NaN similarities: `topk(largest=False)` takes those
    last, and so must k_dycoke_select (it orders a NaN key as +inf when it loads it; without that the bitonic network's comparison is
    no order, kept tokens move and the NaN token itself is kept)."""
    from oracle import dycoke_oracle as D
    from sttm_amd.dycoke_merger import dycoke_ttm
    meta, x, feat, idx = DO.load_dycod(fid)
    T, P = meta["T"], meta["side"] ** 2
    _, _, sims = D.dycoke_ttm(x, T, meta["prune"], return_sims=True)
    out, oi = dycoke_ttm(x.to(DEV), T, meta["prune"])
    DO.check_degenerate(out.cpu(), oi.cpu(), x, idx, sims, T, P, int((1 - meta["prune"]) * P))


# ---- stage 2: group sizes -------------------------------------------------------------------------------------------------------------
def test_scores_at_every_group_size():
    from sttm_amd.dycoke_decode import decode_attn_scores
    _, eps = score_allowance()
    worst = 0.0
    for n, (dt, Hq, Hkv, Dh, Lk) in enumerate(DO.group_cases()):
        q, k, _ = make_qkv(dt, Hq, Hkv, Dh, Lk, n % 2 == 1, 2000 + n)
        got = decode_attn_scores(q, k, Dh ** -0.5)
        assert got.shape == (Lk,) and got.dtype == torch.float32
        err = _rel(got, R.decode_attn_scores_ref(q.double(), k.double(), Dh ** -0.5))
        worst = max(worst, err)
        assert err <= eps, (dt, Hq, Hkv, Dh, Lk, err, eps)
    print(f"scores over the group-size cases: largest relative deviation from float64 {worst:.3e} (allowance {eps:.3e})")


@pytest.mark.parametrize("dname", list(DO.DTYPES))
def test_gathered_attention_at_every_group_size(dname):
    from sttm_amd.dycoke_decode import gathered_decode_attention
    from tests.test_hip_dycoke_decode import _keep_lists
    dt = DO.DTYPES[dname]
    _, tol = attn_allowance(dt)
    worst = 0.0
    for n, (cdt, Hq, Hkv, Dh, Lk) in enumerate(DO.group_cases()):
        if cdt != dt:
            continue
        q, k, v = make_qkv(dt, Hq, Hkv, Dh, Lk, n % 2 == 1, 2100 + n)
        for name, keep in _keep_lists(Lk, n).items():
            got = gathered_decode_attention(q, k, v, keep, Dh ** -0.5)
            assert got.shape == (1, 1, Hq, Dh) and got.dtype == dt
            err = _attn_err(got, R.gathered_decode_attention_ref(q.double(), k.double(), v.double(), keep, Dh ** -0.5))
            worst = max(worst, err)
            assert err <= tol, (dt, Hq, Hkv, Dh, Lk, name, err, tol)
    print(f"gathered attention over the group-size cases, {dt}: largest error {worst:.3e} (allowance {tol:.3e})")


def test_more_than_256_query_heads_raise():
    from sttm_amd.dycoke_decode import decode_attn_scores, gathered_decode_attention
    Hq, Hkv = DO.GROUP_TOO_MANY
    q, k, v = make_qkv(torch.float32, Hq, Hkv, 64, 33, False, 1)
    with pytest.raises(NotImplementedError, match="query heads"):
        decode_attn_scores(q, k, 0.125)
    with pytest.raises(NotImplementedError, match="query heads"):
        gathered_decode_attention(q, k, v, torch.arange(33, dtype=torch.int32, device=DEV), 0.125)


# ---- stage 2: the peaked family -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def peaked_score_allowance():
    base, eps = DO.peaked_score_allowance(DEV)
    print(f"peaked scores, reference-to-reference deviation (float32 on the GPU vs float64): {base:.3e}; kernel allowance {eps:.3e}")
    return base, eps


def _peaked(case):
    dt, Hq, Hkv, Dh, Lk, seed, sigma, sink = case
    return DO.peaked_qkv(dt, Hq, Hkv, Dh, Lk, seed, sigma, sink, DEV)


@functools.lru_cache(maxsize=None)
def peaked_attn_allowance(dt):
    """(largest error of torch's index_select + sdpa in the model dtype against float64 over the peaked cases of that dtype and their
    keep lists, 2 x that), as attn_allowance does for the Gaussian family."""
    worst = 0.0
    for case in DO.PEAKED_CASES:
        if case[0] != dt:
            continue
        _, Hq, Hkv, Dh, Lk = case[:5]
        q, k, v = _peaked(case)
        for keep in DO.peaked_keep_lists(Lk).values():
            idx = keep.to(DEV)
            ref = R.gathered_decode_attention_ref(q.double(), k.double(), v.double(), idx, Dh ** -0.5)
            own = torch.nn.functional.scaled_dot_product_attention(q, k.index_select(2, idx), v.index_select(2, idx), scale=Dh ** -0.5,
                                                                   enable_gqa=True).transpose(1, 2)
            worst = max(worst, _attn_err(own, ref))
    print(f"peaked gathered attention, {dt}: torch index_select + sdpa deviates {worst:.3e} from float64; kernel allowance {2 * worst:.3e}")
    return worst, 2 * worst


def test_peaked_scores_against_float64():
    from sttm_amd.dycoke_decode import decode_attn_scores
    base, eps = peaked_score_allowance()
    worst = 0.0
    for case in DO.PEAKED_CASES + [DO.SATURATED_CASE]:
        dt, Hq, Hkv, Dh, Lk = case[:5]
        q, k, _ = _peaked(case)
        got = decode_attn_scores(q, k, Dh ** -0.5)
        ref = DO.scores64(q, k, Dh)
        live = ref >= DO.FLOOR
        assert bool(live[0]) and (case is DO.SATURATED_CASE or bool(live.all()))
        err = float(((got.double() - ref).abs() / ref)[live].max())
        worst = max(worst, err)
        assert err <= eps, (case, err, eps)
        low = got[~live]                                                       # saturated case only: finite, non-negative, tiny
        assert bool(torch.isfinite(low).all()) and bool((low >= 0).all()) and bool((low <= 2.0 ** -99).all()), case
    print(f"kernel scores, peaked family: largest relative deviation from float64 {worst:.3e} (allowance {eps:.3e}, reference's own {base:.3e})")


def test_peaked_selection_end_to_end_respects_the_threshold_band():
    """The band test of test_selection_end_to_end_respects_the_threshold_band on the peaked family, with a window that leaves the sink
    out (start = 1) and one that holds it."""
    from sttm_amd.dycoke_decode import decode_attn_scores, select_keep
    _, eps = peaked_score_allowance()
    for case in DO.BAND_CASES:
        dt, Hq, Hkv, Dh, Lk = case[:5]
        q, k, _ = _peaked(case)
        score = decode_attn_scores(q, k, Dh ** -0.5)
        s = DO.scores64(q, k, Dh)
        for start in DO.BAND_STARTS:
            n0, num_keep = DO.band_geometry(Lk, start)
            keep = select_keep(score, start, n0, num_keep).long()
            DO.check_keep_well_formed(keep.cpu(), Lk, start, n0, num_keep)
            theta, gap = DO.cut_gap(s, start, n0, num_keep)
            win = s[start:start + n0]
            kept = torch.zeros(Lk, dtype=torch.bool, device=DEV)
            kept[keep] = True
            kw = kept[start:start + n0]
            in_band = int(((win >= theta * (1 - eps)) & (win <= theta * (1 + eps))).sum())
            print(f"peaked end to end {dt} Lk={Lk} start={start}: theta {theta:.3e}, gap {gap:.1e}, {in_band} window entries inside the band")
            assert in_band <= 2, (case, start, in_band)
            assert int(kw.sum()) == num_keep
            assert float(win[kw].min()) >= theta * (1 - eps) and float(win[~kw].max()) <= theta * (1 + eps), (case, start)


@pytest.mark.parametrize("dname", list(DO.DTYPES))
def test_peaked_gathered_attention_against_float64(dname):
    from sttm_amd.dycoke_decode import gathered_decode_attention
    dt = DO.DTYPES[dname]
    base, tol = peaked_attn_allowance(dt)
    worst = 0.0
    for case in DO.PEAKED_CASES:
        if case[0] != dt:
            continue
        _, Hq, Hkv, Dh, Lk = case[:5]
        q, k, v = _peaked(case)
        for name, keep in DO.peaked_keep_lists(Lk).items():
            keep = keep.to(torch.int32).to(DEV)
            got = gathered_decode_attention(q, k, v, keep, Dh ** -0.5)
            err = _attn_err(got, R.gathered_decode_attention_ref(q.double(), k.double(), v.double(), keep, Dh ** -0.5))
            worst = max(worst, err)
            assert err <= tol, (case, name, err, tol)
    print(f"kernel gathered attention, peaked family, {dt}: largest error {worst:.3e} (allowance {tol:.3e}, torch's own {base:.3e})")


def test_non_finite_cache_row():
    """One NaN and one +Inf element in a K row: the scores have the NaN pattern of the float64 restatement (every head's softmax is
    NaN, so all of them), and select_keep on such scores still returns a well-formed list."""
    from sttm_amd.dycoke_decode import decode_attn_scores, select_keep
    for n, (dt, Hq, Hkv, Dh, Lk) in enumerate(((torch.float32, 4, 2, 128, 300), (torch.bfloat16, 12, 1, 64, 257))):
        q, k, _ = make_qkv(dt, Hq, Hkv, Dh, Lk, False, 2300 + n)
        k[0, :, 40, 3] = float("nan")
        k[0, :, 40, 9] = float("inf")
        ref = R.decode_attn_scores_ref(q.double(), k.double(), Dh ** -0.5)
        got = decode_attn_scores(q, k, Dh ** -0.5)
        assert bool(torch.isnan(ref).all()) and torch.equal(torch.isnan(got), torch.isnan(ref))
        for start, n0, num_keep in ((3, 200, 40), (0, Lk, Lk // 5), (5, 400, 0)):
            DO.check_keep_well_formed(select_keep(got, start, n0, num_keep).cpu(), Lk, start, n0, num_keep)


def _lone_qkv(case, n, edit):
    dt, Hq, Hkv, Dh = case
    q, k, v = make_qkv(dt, Hq, Hkv, Dh, DO.LONE_LK, False, 2350 + n)
    for elem, value in DO.LONE_EDITS[edit]:
        k[0, :, DO.LONE_ROW, elem] = value
    return q, k, v


@pytest.mark.parametrize("edit", list(DO.LONE_EDITS))
def test_non_finite_cache_row_alone_in_its_tile_scores(edit):
    """Lk = 257: the non-finite row is the only valid row of the last tile of k_dec_logits, for every dtype and D.  fmaxf drops NaN,
    so that tile's maximum is -inf like a skipped tile's; its NaN must still reach every score, as in the float64 restatement."""
    from sttm_amd.dycoke_decode import decode_attn_scores
    _, eps = score_allowance()
    for n, case in enumerate(DO.lone_cases()):
        Dh = case[3]
        q, k, _ = _lone_qkv(case, n, edit)
        ref = R.decode_attn_scores_ref(q.double(), k.double(), Dh ** -0.5)
        got = decode_attn_scores(q, k, Dh ** -0.5)
        nan = torch.isnan(ref)
        assert edit == "inf" or bool(nan.all())
        assert torch.equal(torch.isnan(got), nan), (case, edit, int(torch.isnan(got).sum()), int(nan.sum()))
        if not bool(nan.all()):                                                # +Inf alone and q's element negative in every head
            fin = ~nan & (ref > 0)
            assert float(((got.double() - ref).abs() / ref)[fin].max()) <= eps and bool((got[~nan & (ref == 0)] == 0).all())


@pytest.mark.parametrize("edit", list(DO.LONE_EDITS))
def test_non_finite_cache_row_alone_in_its_tile_gathered(edit):
    """Keep lists in which one whole tile of k_dec_gathered holds no valid entry but the non-finite row: the output is NaN where the
    float64 attention over the valid ids is (the heads whose logit on that row is NaN or +inf), and within the allowance elsewhere."""
    from sttm_amd.dycoke_decode import gathered_decode_attention
    for n, case in enumerate(DO.lone_cases()):
        dt, Hq, Hkv, Dh = case
        _, tol = attn_allowance(dt)
        q, k, v = _lone_qkv(case, n, edit)
        for name, keep in DO.lone_keep_lists(dt, Dh).items():
            valid = keep[(keep >= 0) & (keep < DO.LONE_LK)].to(DEV)
            ref = R.gathered_decode_attention_ref(q.double(), k.double(), v.double(), valid, Dh ** -0.5)
            got = gathered_decode_attention(q, k, v, keep.to(DEV), Dh ** -0.5)
            nan = torch.isnan(ref)
            assert edit == "inf" or bool(nan.all())
            assert torch.equal(torch.isnan(got), nan), (case, edit, name, int(torch.isnan(got).sum()), int(nan.sum()))
            if not bool(nan.all()):
                err = float((got.double() - ref)[~nan].abs().max() / ref[~nan].abs().max())
                assert err <= tol, (case, edit, name, err, tol)


# ---- stage 2: layouts -----------------------------------------------------------------------------------------------------------------
def _layouts(dt, Hq, Hkv, Dh, Lk, seed):
    """name -> (q, k, v) views of the same logical tensors in awkward storage, plus the plain tensors under "plain"."""
    q, k, v = make_qkv(dt, Hq, Hkv, Dh, Lk, False, seed)
    eb = q.element_size()
    out = {"plain": (q, k, v)}

    def widened(t, width):
        buf = torch.zeros(*t.shape[:-1], width, dtype=dt, device=DEV)
        buf[..., :t.shape[-1]] = t
        return buf[..., :t.shape[-1]]

    def shifted(t):                                                           # storage starts one element past a 16-byte boundary
        buf = torch.zeros(t.numel() + 1, dtype=dt, device=DEV)
        view = buf[1:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == eb
        return view

    odd = Dh + (4 if eb == 2 else 1)                                 # a row stride that is no multiple of 16 bytes
    assert (odd * eb) % 16
    out["row_stride_off_16_bytes"] = (q, widened(k, odd), widened(v, odd))      # the copy path of _rows16
    out["k_storage_shifted"] = (q, shifted(k), v)                              # the copy path of _rows16, K only
    out["k_strided_v_contiguous"] = (q, widened(k, 2 * Dh), v)                 # read in place: k_sl = 2 D, v_sl = D
    out["q_left_half"] = (widened(q, 2 * Dh), k, v)                            # read in place: q_sh = 2 D
    assert out["k_strided_v_contiguous"][1].stride(2) == 2 * Dh and out["q_left_half"][0].stride(1) == 2 * Dh
    return out


@pytest.mark.parametrize("dname,Dh", [("bfloat16", 64), ("float32", 128), ("float16", 128)])
def test_layouts_against_float64(dname, Dh):
    from sttm_amd.dycoke_decode import decode_attn_scores, gathered_decode_attention
    dt = DO.DTYPES[dname]
    Hq, Hkv, Lk = 12, 4, 257
    _, eps = score_allowance()
    _, tol = attn_allowance(dt)
    lay = _layouts(dt, Hq, Hkv, Dh, Lk, 2400)
    q0, k0, v0 = lay["plain"]
    keep = torch.arange(0, Lk, 3, dtype=torch.int32, device=DEV)
    sref = R.decode_attn_scores_ref(q0.double(), k0.double(), Dh ** -0.5)
    aref = R.gathered_decode_attention_ref(q0.double(), k0.double(), v0.double(), keep, Dh ** -0.5)
    for name, (q, k, v) in lay.items():
        assert torch.equal(q, q0) and torch.equal(k, k0) and torch.equal(v, v0)
        err = _rel(decode_attn_scores(q, k, Dh ** -0.5), sref)
        assert err <= eps, (name, err, eps)
        err = _attn_err(gathered_decode_attention(q, k, v, keep, Dh ** -0.5), aref)
        assert err <= tol, (name, err, tol)


# ---- stage 2: skipped keep entries ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A_scattered", "B_whole_tile"])
def test_skipped_keep_entries_contribute_nothing(name):
    """Keep entries outside [0, Lk) are skipped before any load (the range check of k_dec_gathered).  The result is the attention over
    the valid ids alone -- also where a whole tile is skipped: its max is -inf, and dec_tile_softmax gives it probabilities and a sum
    of 0 (it used to store exp(-inf + inf) = NaN, which k_dec_combine spread over the row)."""
    from sttm_amd.dycoke_decode import gathered_decode_attention
    Dh, Lk = 128, DO.SKIP_LK
    _, tol = attn_allowance(torch.float32)
    keep, valid = DO.skip_keep_lists()[name]
    for Hq, Hkv in ((4, 2), (12, 1)):
        q, k, v = make_qkv(torch.float32, Hq, Hkv, Dh, Lk, False, 2500 + Hq)
        got = gathered_decode_attention(q, k, v, keep.to(DEV), Dh ** -0.5)
        ref = R.gathered_decode_attention_ref(q.double(), k.double(), v.double(), valid.to(DEV), Dh ** -0.5)
        assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
        err = _attn_err(got, ref)
        assert err <= tol, (name, Hq, Hkv, err, tol)
