"""The conditions the GPU tests of tests/test_hip_dycoke_offdist.py rest on, checked without a GPU: the oracle against the
reference-made dycod_* fixtures, that the 16-bit width cases have (almost) no token within 2 ulps of a cut, that the peaked family is
as peaked as the tests assume, and the host-side refusals."""
import torch
import pytest

from oracle import dycoke_oracle as D
from sttm_amd import _lib
from tests import _dycoke_decode_ref as R
from tests import _dycoke_offdist as DO


# ---- stage 1 ------------------------------------------------------------------------------------------------------------------------
def test_width_tables_reach_every_branch_of_the_launcher():
    """The branch conditions of launch_dycoke restated on the case tables (the comments next to the tables name the kernels)."""
    def sim32(C):
        return 0 if C % 4 else 4 if C <= 1024 else 8 if C <= 2048 else 16 if C <= 4096 else 0

    assert [sim32(c) for c, _, _ in DO.FP32_WIDTHS] == [4, 8, 8, 16, 16, 16, 0, 0, 0]
    assert [(c % 8 == 0, (c + 511) // 512 if c % 8 == 0 else None, sim32(c // 2)) for c, _, _ in DO.LOWP_WIDTHS] == [
        (True, 1, 4), (True, 2, 4), (True, 2, 4), (True, 7, 8), (True, 9, 16), (False, None, 0), (False, None, 0)]
    assert [(c % 8 == 0, (c + 511) // 512, sim32(c // 2), fam) for c, fam, _ in DO.LOWP_SYNTH_F16] == [
        (True, 7, 8, "synth"), (True, 2, 4, "synth")]
    assert len(DO.LOWP_CASES) == 2 * len(DO.LOWP_WIDTHS) + len(DO.LOWP_SYNTH_F16)
    assert [h * w for h, w in DO.P_EDGES] == [1, 63, 64, 65, 729, 1296, 2048] and DO.P_TOO_MANY[0] * DO.P_TOO_MANY[1] == 2049


@pytest.mark.parametrize("C,family,seed,dname", DO.LOWP_CASES, ids=lambda v: str(v))
def test_lowp_width_cases_have_few_tokens_near_a_cut(C, family, seed, dname):
    """The cap of the GPU test is max(1, near): with near at most 2 % of the kept tokens it cannot hide a wrong trip count.  Also:
    F.cosine_similarity in the input dtype is the oracle's token_cosine bit for bit on these shapes."""
    x, ref = DO.lowp_reference(C, family, seed, dname)
    assert ref.kept == 4 * 24
    print(f"C={C} {dname}: {ref.near} tokens within 2 ulps of a cut, {min(len(set(s.tolist())) for s in ref.sims.values())}+ distinct per frame")
    assert ref.near <= 0.02 * ref.kept, "change the seed of this case"
    fr = x.reshape(DO.WIDTH_T, 49, C)
    for f, s in ref.sims.items():
        assert torch.equal(s, D.token_cosine(fr[D.pruning_partner(f, DO.WIDTH_T)], fr[f]))
    # the stable-sort reference checks itself
    out_idx = torch.cat([ref.keep[f] + f * 49 if f in ref.keep else torch.arange(49) + f * 49 for f in range(DO.WIDTH_T)])
    assert ref.check(x[out_idx], out_idx, x) == 0


def test_too_many_tokens_per_frame_is_refused_before_any_launch():
    """P = 2049 through the C ABI with host pointers.  The workspace size passed is 0, so a call that got past the P check would be
    refused as "workspace too small" (another return code and message): with or without a device nothing is ever launched."""
    lib = _lib.load()
    buf = torch.zeros(64)
    ptr = buf.data_ptr()
    assert lib.sttm_dycoke_ttm(ptr, 5, 2049, 16, _lib.STTM_F32, 1024, ptr, 0, ptr, ptr, None) == _lib.ERR_UNSUPPORTED
    assert "2048 tokens per frame" in _lib.last_error()


@pytest.mark.parametrize("fid", DO.degenerate_ids())
def test_oracle_matches_the_degenerate_vectors(fid):
    meta, x, feat, idx = DO.load_dycod(fid)
    assert DO.bits_equal(x, DO.build_degenerate(meta["case"], meta["dtype"])), "the builder no longer makes the fixture's input"
    f, i, sims = D.dycoke_ttm(x, meta["T"], meta["prune"], return_sims=True)
    assert torch.equal(i, idx) and DO.bits_equal(f, feat)
    P = meta["side"] ** 2
    k = int((1 - meta["prune"]) * P)
    DO.check_degenerate(f, i, x, idx, sims, meta["T"], P, k)                  # the checker accepts the reference's own output
    nonfinite = sum(int((~torch.isfinite(s.float())).sum()) for s in sims.values())
    kept_nonfinite = int((~torch.isfinite(torch.cat([sims[int(t) // P][int(t) % P].float().reshape(1) for t in i if int(t) // P in sims]))).sum())
    print(f"{fid}: {nonfinite} non-finite similarities, {kept_nonfinite} of them kept")
    assert (nonfinite > 0) == (meta["case"] in DO.DEG_NONFINITE)
    assert kept_nonfinite == (49 if meta["case"] == "few_finite" else 0)


def test_degenerate_checker_rejects_what_an_unordered_sort_produces():
    """A kept NaN token in place of a finite one, and a pad id, must both fail the checker."""
    meta, x, feat, idx = DO.load_dycod("dycod_nan_elem_f32")
    P, T = 196, meta["T"]
    k = int((1 - meta["prune"]) * P)
    _, _, sims = D.dycoke_ttm(x, T, meta["prune"], return_sims=True)
    row = P + k + k                                                            # first kept row of frame 3
    bad = idx.clone()
    bad[row + k - 1] = 3 * P + 50                                              # the NaN token
    with pytest.raises(AssertionError, match="non-finite"):
        DO.check_degenerate(x[bad], bad, x, idx, sims, T, P, k)
    bad = idx.clone()
    bad[row] = 3 * P + 0x7fffffff
    with pytest.raises(AssertionError, match="outside the frame"):
        DO.check_degenerate(feat, bad, x, idx, sims, T, P, k)


@pytest.mark.parametrize("fid", DO.degenerate_ids())
def test_select_network_replayed_on_the_cpu_needs_the_nan_rule(fid):
    """k_dycoke_select's network replayed on the oracle's similarities.  With NaN keys loaded as +inf every clip meets the checker;
    with the raw keys the comparison is no order and exactly the clips with a non-finite similarity fail (a NaN token is kept while
    finite ones are left out): those are the GPU tests that fail without the rule."""
    meta, x, feat, idx = DO.load_dycod(fid)
    T, P = meta["T"], meta["side"] ** 2
    k = int((1 - meta["prune"]) * P)
    _, _, sims = D.dycoke_ttm(x, T, meta["prune"], return_sims=True)

    def run(rule):
        ids = torch.cat([DO.replay_select(sims[f].float().numpy(), k, rule) + f * P if f in sims else torch.arange(P) + f * P
                         for f in range(T)])
        DO.check_degenerate(x[ids], ids, x, idx, sims, T, P, k)

    run(True)
    if meta["case"] in DO.DEG_NONFINITE:
        with pytest.raises(AssertionError, match="non-finite similarity kept"):
            run(False)
    else:
        run(False)


# ---- stage 2 ------------------------------------------------------------------------------------------------------------------------
def test_group_cases_cover_the_sweeps():
    cases = DO.group_cases()
    assert len(cases) == 3 * 2 * len(DO.GROUP_HEADS)
    assert sorted({-(-(Hq // Hkv) // 8) for _, Hq, Hkv, _, _ in cases}) == [1, 2, 32]          # sweeps of kDecGmax = 8 heads
    for heads in DO.GROUP_HEADS:
        assert {Lk for _, Hq, Hkv, _, Lk in cases if (Hq, Hkv) == heads} == set(DO.GROUP_LKS)
    lib = _lib.load()
    assert lib.sttm_decode_workspace_bytes(256, 1000, 1000) > 0
    assert lib.sttm_decode_workspace_bytes(DO.GROUP_TOO_MANY[0], 33, 33) == 0 and "query heads" in _lib.last_error()


def test_peaked_family_is_peaked_and_stays_above_the_floor():
    lo, hi, smallest, mass = 0.0, 0.0, [], 0.0
    for dt, Hq, Hkv, Dh, Lk, seed, sigma, sink in DO.PEAKED_CASES:
        q, k, _ = DO.peaked_qkv(dt, Hq, Hkv, Dh, Lk, seed, sigma, sink)
        logits = torch.matmul(q.double(), R.repeat_kv(k.double(), Hq // Hkv).transpose(2, 3)) * Dh ** -0.5
        s = DO.scores64(q, k, Dh)
        lo, hi = min(lo, float(logits.min())), max(hi, float(logits.max()))
        smallest.append(float(s.min()))
        mass = max(mass, float(s[0]))
        spread = float(logits[..., 1:].std())
        assert 0.8 * sigma <= spread <= 1.25 * sigma, (sigma, spread)
        assert float(logits[0, :, 0, 0].max()) > 3 * sigma                       # the sink stands out for at least one head
        assert float(s.min()) >= DO.FLOOR, "a non-saturated case has a score below the floor"
        assert float(logits.max() - logits.min()) > 25.0                      # tile statistics many orders of magnitude apart
    print(f"peaked family: logits in [{lo:.1f}, {hi:.1f}], smallest float64 score {min(smallest):.1e} .. {max(smallest):.1e}, "
          f"the sink holds up to {mass:.2f} of the mass")
    assert min(smallest) < 1e-12 and mass > 0.5
    dt, Hq, Hkv, Dh, Lk, seed, sigma, sink = DO.SATURATED_CASE
    q, k, _ = DO.peaked_qkv(dt, Hq, Hkv, Dh, Lk, seed, sigma, sink)
    sink_logits = torch.matmul(q.double(), k.double()[:, :, :1].transpose(2, 3)).flatten() * Dh ** -0.5
    assert bool(((sink_logits - sink).abs() <= 0.2 * sink).all())              # one head per group: |q| / sqrt(D) = 1 +- 0.09
    s = DO.scores64(q, k, Dh)
    assert float(s[0]) > 0.999 and float(s[1:].max()) < DO.FLOOR              # every other score is below the floor


def test_peaked_allowance_and_the_gap_at_the_cut():
    """The float32 restatement against float64 on this machine, and: the reference's relative gap at the cut of every band case
    exceeds ten times the allowance, so `at most 2 window entries inside the band` is a property of the input."""
    base, eps = DO.peaked_score_allowance()
    print(f"peaked scores, float32 restatement on the CPU vs float64: {base:.3e}; allowance {eps:.3e}")
    assert 0.0 < base < 1e-3
    gaps = []
    for dt, Hq, Hkv, Dh, Lk, seed, sigma, sink in DO.BAND_CASES:
        q, k, _ = DO.peaked_qkv(dt, Hq, Hkv, Dh, Lk, seed, sigma, sink)
        s = DO.scores64(q, k, Dh)
        for start in DO.BAND_STARTS:
            n0, num_keep = DO.band_geometry(Lk, start)
            theta, gap = DO.cut_gap(s, start, n0, num_keep)
            gaps.append(gap)
            assert gap > 10 * eps, (Hq, Hkv, Dh, Lk, sigma, sink, start, gap, eps)
            win = s[start:start + n0]
            assert int(((win >= theta * (1 - eps)) & (win <= theta * (1 + eps))).sum()) == 1
    print(f"relative gap at the cut: {min(gaps):.1e} .. {max(gaps):.1e}")


def test_all_nan_scores_still_select_a_well_formed_list():
    s = torch.full((300,), float("nan"))
    for start, n0, num_keep in ((3, 200, 40), (0, 300, 300), (5, 400, 0)):
        DO.check_keep_well_formed(R.select_keep_ref(s, start, n0, num_keep), 300, start, n0, num_keep)
    with pytest.raises(AssertionError):
        DO.check_keep_well_formed(torch.tensor([0, 1, 2, 9, 8, 203]), 204, 3, 200, 2)


def test_lone_row_cases_put_the_non_finite_row_alone_in_a_tile():
    """Lk = 257 leaves row 256 alone in the last tile of k_dec_logits at every tile height, and each keep list has one tile of
    k_dec_gathered whose only valid entry is that row.  The float64 references are all NaN where the row's logit is NaN."""
    cases = DO.lone_cases()
    assert {(dt, Dh) for dt, _, _, Dh in cases} == {(dt, Dh) for dt in DO.DTYPES.values() for Dh in (64, 128)}
    assert {DO.tile_rows(dt, Dh) for dt, _, _, Dh in cases} == {32, 64, 128}
    ok = lambda t: (t >= 0) & (t < DO.LONE_LK)                                  # noqa: E731
    for n, (dt, Hq, Hkv, Dh) in enumerate(cases):
        rows = DO.tile_rows(dt, Dh)
        assert DO.LONE_LK % rows == 1 and DO.LONE_ROW == DO.LONE_LK - 1
        lists = DO.lone_keep_lists(dt, Dh)
        for name, keep in lists.items():
            tiles = [keep[t:t + rows] for t in range(0, keep.numel(), rows)]
            lone = [t for t in tiles if t[ok(t)].tolist() == [DO.LONE_ROW]]
            assert len(tiles) == 2 and len(lone) == 1, name
            assert int((keep == DO.LONE_ROW).sum()) == 1 and int(ok(keep).sum()) == rows + 1
        g = torch.Generator().manual_seed(n)
        q, k, v = (torch.randn(1, h, l, Dh, generator=g).to(dt).double() for h, l in ((Hq, 1), (Hkv, DO.LONE_LK), (Hkv, DO.LONE_LK)))
        for elem, value in DO.LONE_EDITS["nan_and_inf"]:
            k[0, :, DO.LONE_ROW, elem] = value
        assert bool(torch.isnan(R.decode_attn_scores_ref(q, k, Dh ** -0.5)).all())
        keep = lists["full_tile_then_lone"]
        assert bool(torch.isnan(R.gathered_decode_attention_ref(q, k, v, keep, Dh ** -0.5)).all())


def test_rows16_copies_a_contiguous_tensor_whose_storage_is_off_the_boundary():
    """`.contiguous()` returns a contiguous tensor as it is, wherever its storage starts: the wrapper must copy it itself."""
    from sttm_amd.dycoke_decode import _rows16
    for dt in DO.DTYPES.values():
        buf = torch.arange(2 * 5 * 64 + 1).to(dt)
        t = buf[1:].view(1, 2, 5, 64)
        assert t.is_contiguous() and t.data_ptr() % 16 == t.element_size()
        r = _rows16(t)
        assert r.data_ptr() % 16 == 0 and torch.equal(r, t) and r.stride() == t.stride()
        wide = torch.zeros(1, 2, 5, 68 if t.element_size() == 2 else 65, dtype=dt)[..., :64]       # rows 136 / 260 bytes apart
        assert _rows16(wide).is_contiguous() and _rows16(wide).data_ptr() % 16 == 0
        ok = torch.zeros(1, 2, 5, 128, dtype=dt)[..., :64]
        assert _rows16(ok) is ok                                               # aligned rows are read in place


def test_skip_lists_hold_a_whole_tile_of_skipped_entries():
    lists = DO.skip_keep_lists()
    a, va = lists["A_scattered"]
    b, vb = lists["B_whole_tile"]
    ok = lambda t: (t >= 0) & (t < DO.SKIP_LK)                                  # noqa: E731
    assert int((~ok(a)).sum()) == 5 and torch.equal(a[ok(a)], va) and a.numel() <= DO.SKIP_LK
    # 32 = kDecRpg * 256 / (128 * 4 / 16): the rows of a k_dec_gathered<float, 128> tile
    assert not bool(ok(b[:32]).any()) and torch.equal(b[32:], vb) and bool(ok(vb).all())
