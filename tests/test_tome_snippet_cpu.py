"""CPU-side checks of per-frame / per-snippet ToMe: the restatement against the reference's vectors, the hook glue with the
restatement bound, the two C-ABI entry points and the wrapper's refusals, and the kernel resources of the built library.
No kernel is launched here."""
import os
import re

import pytest
import torch

from tests import _tome_snippet_ref as R
from tests._golden import case_paths, load_case

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sttm_hip.h")


# ---- 1. the restatement is the reference ---------------------------------------------------------------------------------------
def test_fixtures_exist():
    assert len(case_paths(["tsn_"])) >= 4 and len(case_paths(["tsn16_"])) >= 6


@pytest.mark.parametrize("path", case_paths(["tsn_", "tsn16_"]), ids=os.path.basename)
def test_restatement_reproduces_the_reference_vectors(path):
    c = load_case(path)
    m = c["meta"]
    R.assert_no_open_decision(c["x"], m["ratio"], m["S"], m["n_head"], c["name"])
    f, i = R.tome_snippet_ref(c["x"], m["ratio"], m["S"], m["n_head"])
    assert i.dtype == torch.int64 and torch.equal(i, c["idx"]), f"{c['name']}: ids differ"
    assert f.dtype == c["feat"].dtype and torch.equal(f.view(torch.uint8), c["feat"].view(torch.uint8)), f"{c['name']}: features differ"
    T, C, H, W = c["x"].shape
    assert i.numel() == sum(R.snippet_lengths(T, H, W, m["S"], m["ratio"]))


# ---- 2. hook glue -------------------------------------------------------------------------------------------------------------
def _prompt(T, H, W, C, n_sys=5, n_inst=7, seed=0):
    from sttm_amd.synth import synth_video
    vid = synth_video(T, C, H, W, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    hs = torch.cat([torch.randn(1, n_sys, C, generator=g), vid.permute(0, 2, 3, 1).reshape(1, T * H * W, C),
                    torch.randn(1, n_inst, C, generator=g)], dim=1)
    return hs, n_sys, T * H * W


def _bind(cls, calls):
    def fn(video, prune_ratio, snippet_size):
        calls.append((tuple(video.shape), prune_ratio, snippet_size))
        return R.tome_snippet_ref(video, prune_ratio, snippet_size)
    cls.sttm_tome_snippet_fn = staticmethod(fn)


def _unbind(*classes):
    from sttm_amd import monkey_patch_interface as MPI
    MPI.restore_qwen2()
    for cls in classes:
        for name in ("sttm_tome_snippet_fn", "sttm_tome_fn", "sa_tome_snippet_size"):
            if name in cls.__dict__:
                delattr(cls, name)


@pytest.mark.parametrize("S", [1, 2])
def test_qwen2_hook_with_snippet_size(S):
    pytest.importorskip("transformers")
    from transformers import Qwen2Config
    from transformers.models.qwen2.modeling_qwen2 import Qwen2Model
    from oracle import sttm_oracle as O
    from sttm_amd import monkey_patch_interface as MPI
    torch.manual_seed(0)
    C, T, H = 32, 5, 14
    cfg = Qwen2Config(vocab_size=64, hidden_size=C, intermediate_size=64, num_hidden_layers=3, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=4096, attn_implementation="sdpa")
    model = Qwen2Model(cfg).eval()
    hs, start, length = _prompt(T, H, H, C)
    calls = []
    try:
        _bind(Qwen2Model, calls)
        # the default tome_ver is "frame", which raises for T > 1: the snippet size takes its place
        MPI.replace_qwen2_by_sparse_attn("tome", sa_start_layer_idx=1, sa_prune_ratio=0.7, sa_tome_snippet_size=S)
        assert Qwen2Model.sa_tome_snippet_size == S and Qwen2Model.sa_tome_ver == "frame"
        model.image_token_start_index, model.image_token_length, model.num_frame = torch.tensor(start), torch.tensor(length), torch.tensor(T)
        with torch.inference_mode():
            out = model(inputs_embeds=hs, use_cache=False).last_hidden_state
            pos = torch.arange(hs.shape[1]).unsqueeze(0)
            h = model.layers[0](hs, attention_mask=None, position_embeddings=model.rotary_emb(hs, pos), position_ids=pos)
            video = h[0, start:start + length].reshape(T, H, H, C).permute(0, 3, 1, 2)
            tf, tidx = R.tome_snippet_ref(video, 0.7, S)
            h = torch.cat([h[:, :start], tf.unsqueeze(0), h[:, start + length:]], dim=1)
            pos = pos[:, :h.shape[1]]                                  # the LLaVA glue truncates the position ids
            pe = model.rotary_emb(h, pos)
            for layer in model.layers[1:]:
                h = layer(h, attention_mask=None, position_embeddings=pe, position_ids=pos)
            ref = model.norm(h)
        assert calls == [((T, C, H, H), 0.7, S)]
        assert torch.equal(model.merged_token_1d_idx, tidx)
        assert out.shape == ref.shape and out.shape[1] == hs.shape[1] - length + sum(R.snippet_lengths(T, H, H, S, 0.7))
        assert torch.allclose(out, ref, atol=1e-5)
        # installing again without the argument gives today's behaviour: the reference's dispatch, "frame" raises for T > 1
        MPI.replace_qwen2_with_tome_attn(sa_start_layer_idx=1, sa_prune_ratio=0.7)
        assert Qwen2Model.sa_tome_snippet_size is None
        Qwen2Model.sttm_tome_fn = staticmethod(O.get_tome_features)
        with torch.inference_mode(), pytest.raises(RuntimeError):
            model(inputs_embeds=hs, use_cache=False)
        assert len(calls) == 1
    finally:
        _unbind(Qwen2Model)


@pytest.mark.parametrize("S", [1, 2])
def test_qwen2vl_hook_with_snippet_size_gathers_3d_positions(S):
    pytest.importorskip("transformers")
    try:
        from transformers.models.qwen2_vl.configuration_qwen2_vl import Qwen2VLTextConfig
        from transformers.models.qwen2_vl.modeling_qwen2_vl import Qwen2VLTextModel
    except Exception:  # noqa: BLE001
        pytest.skip("this transformers has no Qwen2VLTextModel")
    from transformers.models.qwen2.modeling_qwen2 import Qwen2Model
    from sttm_amd import monkey_patch_interface as MPI
    torch.manual_seed(0)
    C, T, H, W = 32, 3, 10, 18
    cfg = Qwen2VLTextConfig(vocab_size=64, hidden_size=C, intermediate_size=64, num_hidden_layers=3, num_attention_heads=4,
                            num_key_value_heads=2, max_position_embeddings=4096,
                            rope_parameters={"rope_type": "default", "mrope_section": [1, 1, 2], "rope_theta": 10000.0})
    cfg._attn_implementation = "sdpa"
    model = Qwen2VLTextModel(cfg).eval()
    hs, start, length = _prompt(T, H, W, C)
    L = hs.shape[1]
    pos = torch.stack([torch.arange(L), torch.arange(L) // 2, torch.arange(L) // 3]).unsqueeze(1)     # [3, 1, L]
    calls = []
    try:
        _bind(Qwen2VLTextModel, calls)
        MPI.replace_qwen2_by_sparse_attn("tome", sa_start_layer_idx=1, sa_prune_ratio=0.5, sa_tome_snippet_size=S)
        assert Qwen2VLTextModel.sa_tome_snippet_size == S and Qwen2Model.sa_tome_snippet_size == S      # both installers are reached
        model.image_token_start_index, model.image_token_length, model.num_frame = torch.tensor(start), torch.tensor(length), torch.tensor(T)
        model.image_H, model.image_W = torch.tensor(H), torch.tensor(W)
        with torch.inference_mode():
            out = model(inputs_embeds=hs, position_ids=pos, use_cache=False).last_hidden_state
            h = model.layers[0](hs, attention_mask=None, position_embeddings=model.rotary_emb(hs, pos), position_ids=None)
            end = start + length
            video = h[0, start:end].reshape(T, H, W, C).permute(0, 3, 1, 2)
            tf, tidx = R.tome_snippet_ref(video, 0.5, S)
            h = torch.cat([h[:, :start], tf.unsqueeze(0), h[:, end:]], dim=1)
            p2 = torch.cat([pos[:, :, :start], pos[:, :, start:end][:, :, tidx], pos[:, :, end:]], dim=-1)
            pe = model.rotary_emb(h, p2)
            for layer in model.layers[1:]:
                h = layer(h, attention_mask=None, position_embeddings=pe, position_ids=None)
            ref = model.norm(h)
        assert calls == [((T, C, H, W), 0.5, S)]
        assert torch.equal(model.merged_token_1d_idx, tidx)
        # one iteration at ratio 0.5: every snippet keeps exactly its odd tokens, in order
        expect = torch.cat([torch.arange(1, (t1 - t0) * H * W, 2) + t0 * H * W for t0, t1 in R.snippet_ranges(T, S)])
        assert torch.equal(tidx, expect)
        assert out.shape == ref.shape and out.shape[1] == L - length + tidx.numel()
        assert torch.allclose(out, ref, atol=1e-5)
        MPI.replace_qwen2vl_with_tome_attn(sa_start_layer_idx=1, sa_prune_ratio=0.5, sa_tome_snippet_size=None)
        assert Qwen2VLTextModel.sa_tome_snippet_size is None
    finally:
        _unbind(Qwen2VLTextModel, Qwen2Model)


def test_installer_refuses_a_bad_snippet_size():
    pytest.importorskip("transformers")
    from transformers.models.qwen2.modeling_qwen2 import Qwen2Model
    from sttm_amd import monkey_patch_interface as MPI
    try:
        for bad in (0, -1, 1.5, "2", True):
            with pytest.raises((ValueError, TypeError)):
                MPI.replace_qwen2_with_tome_attn(sa_tome_snippet_size=bad)
    finally:
        _unbind(Qwen2Model)


# ---- 3. ABI and wrapper -------------------------------------------------------------------------------------------------------
def test_abi_has_the_two_entry_points():
    from sttm_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in ("sttm_tome_segments_workspace_bytes", "sttm_tome_step_segments"):
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} is not declared in include/sttm_hip.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["sttm_tome_segments_workspace_bytes"][1]) == 4
    assert len(_lib.SIGNATURES["sttm_tome_step_segments"][1]) == 15
    assert lib.sttm_abi_version() == _lib.ABI_VERSION == 8
    cap = int(re.search(r"#define STTM_TOME_SEGMENT_MAX_TOKENS (\d+)", open(HDR).read()).group(1))
    assert cap == _lib.TOME_SEGMENT_MAX_TOKENS >= 784


def test_workspace_bytes_answers_and_refusals():
    from sttm_amd import _lib
    lib = _lib.load()
    cap = _lib.TOME_SEGMENT_MAX_TOKENS
    for n_seg, n, C, h in [(128, 196, 1024, 1), (32, 784, 1024, 1), (128, 196, 3584, 1), (3, 49, 1000, 1), (4, 729, 256, 1), (1, 720, 256, 4),
                           (1, 2, 8, 1), (7, cap, 64, 1)]:
        b = lib.sttm_tome_segments_workspace_bytes(n_seg, n, C, h)
        # at least the unit rows of both halves (two bytes per element) and the per-token bookkeeping
        assert b >= n_seg * n * (C // h) * 2 + n_seg * n * 4, (n_seg, n, C, h)
    assert lib.sttm_tome_segments_workspace_bytes(2, 196, 64, 1) > lib.sttm_tome_segments_workspace_bytes(1, 196, 64, 1)
    for args, word in [((0, 196, 64, 1), "bad"), ((4, 1, 64, 1), "bad"), ((4, 196, 0, 1), "bad"), ((4, 196, 64, 0), "bad"),
                       ((4, 196, 64, 3), "bad"), ((-1, 196, 64, 1), "bad"), ((1, cap + 1, 64, 1), str(cap)), ((4, 4 * 729, 64, 1), str(cap))]:
        assert lib.sttm_tome_segments_workspace_bytes(*args) == 0, args
        assert word in _lib.last_error(), (args, _lib.last_error())


def test_step_refuses_bad_arguments_without_launching():
    from sttm_amd import _lib
    lib = _lib.load()
    p = 4096                      # never dereferenced: every call below is refused on the host
    ok = lib.sttm_tome_segments_workspace_bytes(2, 196, 64, 1)
    call = lambda **kw: lib.sttm_tome_step_segments(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("x", p), ("size", None), ("idx", None), ("n_seg", 2), ("n", 196), ("C", 64), ("n_head", 1), ("r", 98), ("dtype", 0), ("ws", p),
        ("ws_bytes", ok), ("x_out", p), ("size_out", p), ("idx_out", p), ("stream", None))])
    assert call(x=None) == _lib.ERR_ARG and call(ws=None) == _lib.ERR_ARG and call(idx_out=None) == _lib.ERR_ARG
    assert call(dtype=3) == _lib.ERR_ARG and call(r=0) == _lib.ERR_ARG and call(r=99) == _lib.ERR_ARG
    assert call(ws_bytes=ok - 1) == _lib.ERR_ARG and "workspace" in _lib.last_error()
    assert call(n=_lib.TOME_SEGMENT_MAX_TOKENS + 2, r=1) == _lib.ERR_UNSUPPORTED
    assert call(n_seg=0) == _lib.ERR_ARG


def test_wrapper_refusals():
    import sttm_amd
    from sttm_amd import get_tome_features, get_tome_features_batch, get_tome_features_snippet
    assert "get_tome_features_snippet" in sttm_amd.__all__
    x = torch.zeros(4, 16, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        get_tome_features_snippet(x, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        get_tome_features_snippet(x, 0.5, 8)                       # S >= T routes to the per-clip path, which refuses as well
    for bad in (0, -3, 1.5, "1", None, True):
        with pytest.raises(ValueError):
            get_tome_features_snippet(x, 0.5, bad)
    # the reference's dispatch is unchanged: "frame" raises for T > 1, "snippet" and unknown versions return None
    with pytest.raises(RuntimeError, match="frame"):
        get_tome_features(x, 0.5, "frame")
    assert get_tome_features(x, 0.5, "snippet") is None and get_tome_features(x, 0.5, "nonsense") is None
    assert get_tome_features_batch([x, x], 0.5, "snippet") == [None, None]


# ---- 4. kernel resources ------------------------------------------------------------------------------------------------------
# the instantiations that serve fp32 C = 1024 and bf16 C = 3584 at 14 x 14 (one head, aligned rows), by mangled name
NO_SCRATCH = [
    ("normalise, fp32 -> two fp16 planes, 16-byte loads", r"k_tsn_normalizeIfLi4E"),
    ("normalise, bf16, 16-byte packs", r"k_tsn_normalizeINS_6bf16_tELi8E"),
    ("match, fp32 as two fp16 planes, three products", r"k_tsn_matchINS_5f16_tELi2ELi3E"),
    ("match, bf16", r"k_tsn_matchINS_6bf16_tELi1ELi1E"),
    ("match, fp16", r"k_tsn_matchINS_5f16_tELi1ELi1E"),
    ("rank + source lists", r"k_tsn_rankE"),
    ("merge, fp32, 16-byte packs", r"k_tsn_mergeIfLi4E"),
    ("merge, bf16, 16-byte packs", r"k_tsn_mergeINS_6bf16_tELi8E"),
]


@pytest.fixture(scope="module")
def kernels():
    from tests.test_kernel_resources import LLVM, _kernels_of
    lib = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sttm_amd", "lib", "libsttm_hip.so")
    assert os.path.exists(lib), "library not built"
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(f"{LLVM}/{tool}"):
            pytest.skip(f"{tool} not available")
    k = _kernels_of(lib)
    assert len(k) > 50, "could not read the kernel descriptors of the library"
    return k


@pytest.mark.parametrize("what,pattern", NO_SCRATCH, ids=[w for w, _ in NO_SCRATCH])
def test_segment_kernels_use_no_scratch(kernels, what, pattern):
    hits = {n: v for n, v in kernels.items() if re.search(pattern, n)}
    assert hits, f"no kernel matches {pattern!r} ({what})"
    spilled = {n: v for n, v in hits.items() if v[0] != 0}
    assert not spilled, f"{what}: scratch in use (bytes per lane, VGPRs): {spilled}"
