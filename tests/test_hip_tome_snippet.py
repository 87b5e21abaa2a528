"""GPU tests of per-frame / per-snippet ToMe (sttm_amd.get_tome_features_snippet, csrc/tome_snippet.hip) against the per-snippet
restatement on the oracle (tests/_tome_snippet_ref.py) and the reference's vectors (tests/golden/tsn_*.npz, tsn16_*.npz).

fp32 fixtures and oracle cases hold no open decision (asserted on the CPU first), so they are compared without slack.  The
full-size clips do hold near-ties: there the bound is one near-tie per snippet that the CPU check flags, zero for all others.

16-bit measurements (MI355X, this file's cases; ids differing / rows beyond 2 ulp, of the call's kept count):
    tsn16_bf16_s1_070 0 / 0 of 236     tsn16_bf16_s2_085 0 / 0 of 177     tsn16_bf16_s1_030 0 / 0 of 552
    tsn16_bf16_s1_060_odd 0 / 0 of 100     tsn16_f16_s1_070 0 / 0 of 236     tsn16_f16_s2_085 0 / 0 of 177
    bf16 T = 128, C = 3584, S = 1, p = 0.7: 12 / 24 of 7 552 (`_assert_tome16` allows 16 / 38 there)
The fixtures are pinned at their counts plus one tie (1 id, 2 rows: `_assert_tome16`'s floor), the full-size clip at 13 / 26.  Its
disagreements are ties of rounded bf16 scores at a snippet's cut or argmax, which the CPU's accumulation order decides the other way
(128 snippets x 2 iterations, C = 3584); the segment kernels' scores are those of the per-clip 128-tile kernel, bit for bit.
"""
import os

import pytest
import torch

from tests import _tome_snippet_ref as R
from tests._golden import case_paths, load_case
from tests.test_hip_parity import FP32_TOL, _assert_tome16, _compare_tome, _tome16_agreement

pytestmark = pytest.mark.gpu

# measured 16-bit disagreements (see the module docstring) plus one tie
PIN16_IDS, PIN16_ROWS = 0 + 1, 0 + 2

FP32_ORACLE_CASES = [  # synth_video(T, C, H, W, seed); S, p, n_head -- verified to hold no open decision
    (8, 1024, 14, 14, 58, 1, 0.5, 1), (8, 1024, 14, 14, 58, 1, 0.7, 1), (16, 1024, 14, 14, 66, 1, 0.85, 1),
    (7, 512, 14, 14, 300, 2, 0.7, 4), (9, 256, 13, 24, 300, 4, 0.6, 1), (6, 256, 20, 36, 316, 1, 0.7, 1),
    (10, 64, 14, 14, 300, 3, 0.85, 1), (5, 1000, 7, 7, 300, 1, 0.3, 1), (3, 256, 27, 27, 303, 1, 0.5, 1),
    (4, 256, 27, 27, 300, 2, 0.7, 1)]


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _structure(x, feat, idx, S, p):
    """Output length, dtype, and the ids of every snippet: in its own range, distinct, all odd local ids kept when one iteration
    suffices.  Returns the per-snippet (start, end) offsets into the output."""
    T, C, H, W = x.shape
    hw = H * W
    lens = R.snippet_lengths(T, H, W, S, p)
    assert feat.shape == (sum(lens), C) and idx.shape == (sum(lens),) and idx.dtype == torch.int64 and feat.dtype == x.dtype
    ic = idx.cpu()
    offs, o = [], 0
    for (t0, t1), n_g in zip(R.snippet_ranges(T, S), lens):
        ids = ic[o:o + n_g]
        assert int(ids.min()) >= t0 * hw and int(ids.max()) < t1 * hw, f"snippet at frame {t0}: ids outside its range"
        assert ids.unique().numel() == n_g, f"snippet at frame {t0}: repeated ids"
        if p <= 0.5:
            odd = torch.arange(1, (t1 - t0) * hw, 2) + t0 * hw
            assert torch.isin(odd, ids).all(), f"snippet at frame {t0}: an odd token is missing after one iteration"
        offs.append((o, o + n_g))
        o += n_g
    return offs


def _exact(x, S, p, n_head, what):
    from sttm_amd import get_tome_features_snippet
    R.assert_no_open_decision(x, p, S, n_head, what)
    ef, ei = R.tome_snippet_ref(x, p, S, n_head)
    f, i = get_tome_features_snippet(x.to(_dev()), p, S, n_head)
    _structure(x, f, i, S, p)
    _compare_tome(f, i, ef, ei, FP32_TOL, what, max_ids=0, max_rows=0)
    if p == 0.5 and (x.shape[2] * x.shape[3]) % 2 == 0:
        assert torch.equal(i.cpu(), ei), f"{what}: r = n/2 keeps exactly the odd tokens, in order"
    return f, i, ef, ei


@pytest.mark.parametrize("path", case_paths(["tsn_"]), ids=os.path.basename)
def test_fp32_reference_vectors(path):
    c = load_case(path)
    m = c["meta"]
    f, i, ef, ei = _exact(c["x"], m["S"], m["ratio"], m["n_head"], c["name"])
    assert torch.equal(ei, c["idx"]) and torch.equal(ef, c["feat"])           # the restatement is the reference (CPU test 1)


@pytest.mark.parametrize("T,C,H,W,seed,S,p,n_head", FP32_ORACLE_CASES)
def test_fp32_against_the_restatement(T, C, H, W, seed, S, p, n_head):
    from sttm_amd.synth import synth_video
    _exact(synth_video(T, C, H, W, seed=seed), S, p, n_head, f"T={T} C={C} {H}x{W} S={S} p={p} heads={n_head}")


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("p", [0.5, 0.7])
def test_full_size_fp32(S, p):
    """T = 128, 14 x 14, C = 1024: one near-tie (`_compare_tome`'s max_ids = 1, max_rows = 2) per snippet that the CPU check flags as
    holding a margin below 1e-5, zero for every other snippet; at most a quarter of the snippets may be flagged."""
    from sttm_amd import get_tome_features_snippet
    from sttm_amd.synth import synth_video
    x = synth_video(128, 1024, 14, 14, seed=178)
    flagged = set(R.open_snippets(x, p, S, 1))
    n_snip = len(R.snippet_ranges(128, S))
    print(f"S={S} p={p}: {len(flagged)} of {n_snip} snippets hold a margin below {R.OPEN_MARGIN}")
    assert len(flagged) <= 0.25 * n_snip
    ef, ei = R.tome_snippet_ref(x, p, S, 1)
    f, i = get_tome_features_snippet(x.to(_dev()), p, S, 1)
    offs = _structure(x, f, i, S, p)
    fc, ic = f.cpu(), i.cpu()
    for g, (a, b) in enumerate(offs):
        slack = (1, 2) if g in flagged else (0, 0)
        _compare_tome(fc[a:b], ic[a:b], ef[a:b], ei[a:b], FP32_TOL, f"S={S} p={p} snippet {g}", max_ids=slack[0], max_rows=slack[1])


def _check16(f, i, ef, ei, what):
    ida, fa = _tome16_agreement(f, i, ef, ei, what)
    n = ei.numel()
    print(f"{what}: {round((1 - ida) * n)} ids differ, {round((1 - fa) * n)} rows beyond 2 ulp, of {n}")
    _assert_tome16(ida, fa, n, what)
    assert round((1 - ida) * n) <= PIN16_IDS and round((1 - fa) * n) <= PIN16_ROWS, f"{what}: above the measured counts plus one tie"


@pytest.mark.parametrize("path", case_paths(["tsn16_"]), ids=os.path.basename)
def test_16bit_reference_vectors(path):
    from sttm_amd import get_tome_features_snippet
    c = load_case(path)
    m = c["meta"]
    R.assert_no_open_decision(c["x"], m["ratio"], m["S"], m["n_head"], c["name"])
    f, i = get_tome_features_snippet(c["x"].to(_dev()), m["ratio"], m["S"], m["n_head"])
    _structure(c["x"], f, i, m["S"], m["ratio"])
    _check16(f, i, c["feat"], c["idx"], c["name"])


def test_full_size_bf16():
    from sttm_amd import get_tome_features_snippet
    from sttm_amd.synth import synth_video
    x = synth_video(128, 3584, 14, 14, seed=178, dtype=torch.bfloat16)
    ef, ei = R.tome_snippet_ref(x, 0.7, 1, 1)
    f, i = get_tome_features_snippet(x.to(_dev()), 0.7, 1, 1)
    _structure(x, f, i, 1, 0.7)
    ida, fa = _tome16_agreement(f, i, ef, ei, "bf16 T=128 C=3584 S=1 p=0.7")
    n = ei.numel()
    print(f"bf16 full size: {round((1 - ida) * n)} ids differ, {round((1 - fa) * n)} rows beyond 2 ulp, of {n}")
    _assert_tome16(ida, fa, n, "bf16 T=128 C=3584 S=1 p=0.7")
    assert round((1 - ida) * n) <= 12 + 1 and round((1 - fa) * n) <= 24 + 2, "above the measured counts plus one tie"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_routes_and_ragged_tails(dtype):
    """S >= T and snippets above the kernels' cap are bit-identical to the "video" calls they route to; ragged tails."""
    from sttm_amd import _lib, get_tome_features, get_tome_features_snippet
    from sttm_amd.synth import synth_video
    dev = _dev()
    x = synth_video(7, 128, 14, 14, seed=41, dtype=dtype).to(dev)
    for S in (7, 9):
        f, i = get_tome_features_snippet(x, 0.7, S)
        ef, ei = get_tome_features(x, 0.7, "video")
        assert torch.equal(i, ei) and torch.equal(f.view(torch.uint8), ef.view(torch.uint8))
    S = 6                                                        # 1176 tokens per snippet: above the cap, with a one-frame tail
    assert S * 196 > _lib.TOME_SEGMENT_MAX_TOKENS
    f, i = get_tome_features_snippet(x, 0.7, S)
    parts = [get_tome_features(x[t0:t1], 0.7, "video") for t0, t1 in R.snippet_ranges(7, S)]
    ef = torch.cat([q[0] for q in parts])
    ei = torch.cat([q[1] + t0 * 196 for q, (t0, _t1) in zip(parts, R.snippet_ranges(7, S))])
    assert torch.equal(i, ei) and torch.equal(f.view(torch.uint8), ef.view(torch.uint8))
    for S, p in [(2, 0.5), (3, 0.85), (4, 0.3), (5, 0.6)]:       # tails of 1, 1, 3 and 2 frames
        f, i = get_tome_features_snippet(x, p, S)
        _structure(x.cpu(), f, i, S, p)
    # a snippet through the segment kernels equals the per-clip path on the same sub-video where nothing is near a tie
    if dtype == torch.float32:
        f, i = get_tome_features_snippet(x, 0.5, 2)
        for (t0, t1), (a, b) in zip(R.snippet_ranges(7, 2), _structure(x.cpu(), f, i, 2, 0.5)):
            ef, ei = get_tome_features(x[t0:t1], 0.5, "video")
            assert torch.equal(i[a:b], ei + t0 * 196)
            assert float((f[a:b] - ef).abs().max()) <= FP32_TOL


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_degenerate_rows(dtype):
    """A NaN row (a zero token has a 0/0 unit row) and a constant frame: valid ids everywhere, finite outputs in the other snippets."""
    from sttm_amd import get_tome_features_snippet
    from sttm_amd.synth import synth_video
    x = synth_video(6, 128, 14, 14, seed=77, dtype=dtype).to(_dev())
    flat = x.permute(0, 2, 3, 1)
    flat[1, 3, 4] = 0
    flat[4] = flat[4, 0, 0]
    for S, p in [(1, 0.7), (2, 0.85), (1, 0.5)]:
        f, i = get_tome_features_snippet(x, p, S)
        offs = _structure(x.cpu(), f, i, S, p)
        for g, (a, b) in enumerate(offs):
            if g != 1 // S:
                assert torch.isfinite(f[a:b].float()).all(), f"S={S} p={p}: snippet {g} is not finite"


def test_errors_on_device():
    from sttm_amd import get_tome_features_snippet
    x = torch.zeros(4, 16, 4, 4, device=_dev())
    with pytest.raises(TypeError):
        get_tome_features_snippet(x + 1, 0.0, 1)
    with pytest.raises(NotImplementedError):
        get_tome_features_snippet(x.double(), 0.5, 1)
    with pytest.raises(ValueError):
        get_tome_features_snippet(x, 0.5, 1.5)


def _tiny_models():
    from transformers import Qwen2Config
    from transformers.models.qwen2.modeling_qwen2 import Qwen2Model
    from transformers.models.qwen2_vl.configuration_qwen2_vl import Qwen2VLTextConfig
    from transformers.models.qwen2_vl.modeling_qwen2_vl import Qwen2VLTextModel
    C = 64
    torch.manual_seed(0)
    cfg = Qwen2Config(vocab_size=64, hidden_size=C, intermediate_size=128, num_hidden_layers=3, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=4096, attn_implementation="sdpa")
    vcfg = Qwen2VLTextConfig(vocab_size=64, hidden_size=C, intermediate_size=128, num_hidden_layers=3, num_attention_heads=4,
                             num_key_value_heads=2, max_position_embeddings=4096,
                             rope_parameters={"rope_type": "default", "mrope_section": [2, 2, 4], "rope_theta": 10000.0})
    vcfg._attn_implementation = "sdpa"
    return Qwen2Model(cfg).eval(), Qwen2VLTextModel(vcfg).eval()


@pytest.mark.parametrize("S", [1, 4])
def test_installed_hook_on_device_equals_the_cpu_bound_hook(S):
    """The installed ToMe hook with sa_tome_snippet_size on the tiny Qwen2 / Qwen2-VL text models: the forward on the device through
    the HIP path equals the same patched forward on the CPU with the restatement bound to sttm_tome_snippet_fn."""
    pytest.importorskip("transformers")
    from sttm_amd import monkey_patch_interface as MPI
    from sttm_amd.synth import synth_video
    dev = _dev()
    T, C, H, W = 6, 64, 12, 12            # square frames: the Qwen2 (LLaVA) glue derives H = W from the token count
    qwen2, qwen2vl = _tiny_models()
    vid = synth_video(T, C, H, W, seed=21)
    g = torch.Generator().manual_seed(22)
    hs = torch.cat([torch.randn(1, 7, C, generator=g), vid.permute(0, 2, 3, 1).reshape(1, T * H * W, C), torch.randn(1, 11, C, generator=g)], dim=1)
    start, length, L = 7, T * H * W, hs.shape[1]
    pos3 = torch.stack([torch.arange(L), torch.arange(L) // 2, torch.arange(L) // 3]).unsqueeze(1)
    for model, kw in ((qwen2, {}), (qwen2vl, dict(position_ids=pos3))):
        cls = type(model)
        outs, idxs = [], []
        for device, fn in (("cpu", staticmethod(lambda v, p, s: R.tome_snippet_ref(v, p, s))), (dev, None)):
            try:
                if fn is not None:
                    cls.sttm_tome_snippet_fn = fn
                MPI.replace_qwen2_by_sparse_attn("tome", sa_start_layer_idx=1, sa_prune_ratio=0.5, sa_tome_snippet_size=S)
                m = model.to(device)
                m.image_token_start_index, m.image_token_length, m.num_frame = torch.tensor(start), torch.tensor(length), torch.tensor(T)
                m.image_H, m.image_W = torch.tensor(H), torch.tensor(W)
                with torch.inference_mode():
                    k = {n: v.to(device) for n, v in kw.items()}
                    outs.append(m(inputs_embeds=hs.to(device), use_cache=False, **k).last_hidden_state.cpu())
                idxs.append(m.merged_token_1d_idx.cpu())
            finally:
                MPI.restore_qwen2()
                if "sttm_tome_snippet_fn" in cls.__dict__:
                    del cls.sttm_tome_snippet_fn
        assert torch.equal(idxs[0], idxs[1])                      # ratio 0.5: the odd tokens of every snippet, in order
        assert outs[0].shape == outs[1].shape and outs[0].shape[1] == L - length + sum(R.snippet_lengths(T, H, W, S, 0.5))
        assert torch.allclose(outs[0], outs[1], atol=2e-5)
