"""DyCoke stage 2 without a GPU: the patched forward with its three injection points bound to the torch restatement
(tests/_dycoke_decode_ref.py) against the decoder layers run by hand, the refusals, the C ABI and the kernels' descriptors."""
import os
import re

import pytest
import torch

from oracle import dycoke_oracle
from sttm_amd import _lib
from sttm_amd import monkey_patch_interface as MPI
from tests import _dycoke_decode_ref as R
from tests._batched_common import prompt_rows, qwen2_model, set_one

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = (3, 6, 3, 3, 4)             # n_sys, T, H, W, n_inst: 54 visual tokens, 34 after stage 1 at prune ratio 0.5
SPEC_TAIL = (3, 6, 3, 3, 30)       # instruction longer than n0 - merged = 20: the tail [start + n0, Lk) is not empty
PRUNE = 0.5
_FNS = ("sttm_dycoke_fn",) + MPI._DECODE_FNS


def _qwen2_cls():
    from transformers.models.qwen2.modeling_qwen2 import Qwen2Model
    return Qwen2Model


def _clean(cls):
    MPI.restore_qwen2()
    for name in _FNS:
        if name in cls.__dict__:
            delattr(cls, name)


def _install(record=None, stage1_only=False, **kw):
    cls = _qwen2_cls()
    if stage1_only:
        MPI.replace_qwen2_by_sparse_attn("dycoke-stage1", sa_start_layer_idx=kw.get("sa_start_layer_idx", 0), sa_prune_ratio=PRUNE)
    else:
        MPI.replace_qwen2_with_dycoke_attn(**{"sa_prune_ratio": PRUNE, "dycoke_l": 2, **kw})
        for name, fn in zip(MPI._DECODE_FNS, R.as_decode_fns(record)):
            setattr(cls, name, staticmethod(fn))
    cls.sttm_dycoke_fn = staticmethod(dycoke_oracle.dycoke_ttm)
    return cls


def _manual_decode_step(model, h, pos, cache, l, start, n0, num_keep):
    """One decode step with the layers run by hand: full cache below layer l, the restatement's keep list from layer l on."""
    from transformers.models.qwen2.modeling_qwen2 import apply_rotary_pos_emb
    cos, sin = model.rotary_emb(h, pos)
    keep = None
    for i, layer in enumerate(model.layers):
        att = layer.self_attn
        x = layer.input_layernorm(h)
        shape = (1, 1, -1, att.head_dim)
        q, k, v = (p(x).view(shape).transpose(1, 2) for p in (att.q_proj, att.k_proj, att.v_proj))
        q, k = apply_rotary_pos_emb(q, k, cos, sin)
        K, V = cache.update(k, v, i)
        if i == l - 1:
            keep = R.select_keep_ref(R.decode_attn_scores_ref(q, K, att.scaling), start, n0, num_keep)
        if i >= l:
            K, V = K[:, :, keep], V[:, :, keep]
        G = q.shape[1] // K.shape[1]
        w = torch.softmax(torch.matmul(q, R.repeat_kv(K, G).transpose(2, 3)) * att.scaling, dim=-1)
        o = torch.matmul(w, R.repeat_kv(V, G)).transpose(1, 2).reshape(1, 1, -1)
        h = h + att.o_proj(o)
        h = h + layer.mlp(layer.post_attention_layernorm(h))
    return model.norm(h), keep


def _run(spec, attn, layers, p, steps=3, sa_start=0, l=2):
    """(hidden states of the patched decode steps, those of the by-hand steps, keep lists of both, the two caches, geometry)."""
    from transformers.cache_utils import DynamicCache
    model = qwen2_model(layers=layers, attn=attn)
    C = model.config.hidden_size
    hs = prompt_rows([spec], C)[0].unsqueeze(0)
    start, n0 = spec[0], spec[1] * spec[2] * spec[3]
    set_one(model, spec)
    g = torch.Generator().manual_seed(5)
    new = [torch.randn(1, 1, C, generator=g) for _ in range(steps)]
    cls = _qwen2_cls()
    rec, got, ref, ref_keeps = [], [], [], []
    try:
        with torch.inference_mode():
            # by hand: the prefill is the existing stage-1 pattern, the decode steps are run layer by layer
            _install(stage1_only=True, sa_start_layer_idx=sa_start)
            cache_ref = DynamicCache(config=model.config)
            model(inputs_embeds=hs, past_key_values=cache_ref, use_cache=True)
            _clean(cls)
            Lp = cache_ref.get_seq_length(l)
            num_keep = R.num_keep_of(n0, p)
            for s, x in enumerate(new):
                out, keep = _manual_decode_step(model, x, torch.tensor([[Lp + s]]), cache_ref, l, start, n0, num_keep)
                ref.append(out)
                ref_keeps.append(keep)
            # the patched forward
            _install(rec, sa_start_layer_idx=sa_start, dycoke_l=l, dycoke_p=p)
            cache = DynamicCache(config=model.config)
            model(inputs_embeds=hs, past_key_values=cache, use_cache=True)
            assert cache.sttm_dycoke == (start, n0) and not rec                      # no selection at prefill
            for s, x in enumerate(new):
                got.append(model(inputs_embeds=x, position_ids=torch.tensor([[Lp + s]]), past_key_values=cache,
                                 use_cache=True).last_hidden_state)
                assert model.config._attn_implementation == attn and model.config._sttm_dycoke_step is None
    finally:
        _clean(cls)
    return got, ref, rec, ref_keeps, cache, cache_ref, (start, n0, Lp)


@pytest.mark.parametrize("attn", ["sdpa", "eager"])
@pytest.mark.parametrize("spec,layers,sa_start", [(SPEC, 3, 0), (SPEC_TAIL, 4, 1)])
def test_patched_decode_matches_layers_by_hand(attn, spec, layers, sa_start):
    p = 0.8
    got, ref, rec, ref_keeps, cache, cache_ref, (start, n0, Lp) = _run(spec, attn, layers, p, sa_start=sa_start)
    num_keep = int(n0 * (1 - p))
    assert len(got) == len(ref) == len(rec) == 3
    for s in range(3):
        assert torch.allclose(got[s], ref[s], atol=1e-5), float((got[s] - ref[s]).abs().max())
        Lk = Lp + s + 1
        tail = max(Lk - start - n0, 0)
        keep = rec[s].tolist()
        assert len(keep) == start + num_keep + tail and len(set(keep)) == len(keep)
        assert set(keep) <= set(range(Lk)) and keep[:start] == list(range(start))
        assert keep == ref_keeps[s].tolist()
        if spec is SPEC_TAIL:
            assert tail > 0 and keep[-tail:] == list(range(start + n0, Lk))
        else:
            assert tail == 0
    # the cache is never shortened: every layer from the merge layer on holds all Lk rows after the last step
    for i in range(layers):
        want = Lp + 3 if i >= sa_start else cache.get_seq_length(0)
        assert cache.get_seq_length(i) == want == cache_ref.get_seq_length(i)
    assert num_keep < Lp - start              # the selection really drops keys


def test_num_keep_above_the_window_raises():
    with pytest.raises(RuntimeError, match="out of range"):
        _run(SPEC, "sdpa", 3, 0.1, steps=1)          # num_keep = 48 of a window of 39 scores


def _decode_once(model, **inputs):
    """Prefill + one decode forward of an installed model; returns the exception the decode step raises, if any."""
    from transformers.cache_utils import DynamicCache
    C = model.config.hidden_size
    hs = prompt_rows([SPEC], C)[0].unsqueeze(0)
    set_one(model, SPEC)
    with torch.inference_mode():
        cache = DynamicCache(config=model.config)
        model(inputs_embeds=hs, past_key_values=cache, use_cache=True)
        return model(inputs_embeds=inputs.get("x", torch.zeros(1, 1, C)), past_key_values=cache, use_cache=True)


def test_refusals_name_their_limit():
    cls = _qwen2_cls()
    try:
        with pytest.raises(ValueError, match="dycoke_l"):
            MPI.replace_qwen2_with_dycoke_attn(dycoke_l=0)
        with pytest.raises(ValueError, match="dycoke_p"):
            MPI.replace_qwen2_with_dycoke_attn(dycoke_p=1.5)
        with pytest.raises(ValueError, match="dycoke_p"):
            MPI.replace_qwen2_with_dycoke_attn(dycoke_p=-0.1)
        assert "_sttm_original_forward" not in cls.__dict__                          # a refused install leaves nothing behind
        _install(dycoke_l=3)
        with pytest.raises(ValueError, match="num_hidden_layers"):
            _decode_once(qwen2_model(layers=3))
        _clean(cls)
        _install(dycoke_l=1, sa_start_layer_idx=1)
        with pytest.raises(ValueError, match="sa_start_layer_idx"):
            _decode_once(qwen2_model(layers=3))
        _clean(cls)
        # batch size above 1, at prefill and at a decode step
        from transformers.cache_utils import DynamicCache
        _install()
        model = qwen2_model(layers=3)
        hs = prompt_rows([SPEC], 32)[0].unsqueeze(0)
        set_one(model, SPEC)
        with torch.inference_mode():
            with pytest.raises(NotImplementedError, match="batch size 1"):
                model(inputs_embeds=hs.repeat(2, 1, 1), use_cache=True)
            cache = DynamicCache(config=model.config)
            model(inputs_embeds=hs, past_key_values=cache, use_cache=True)
            with pytest.raises(NotImplementedError, match="batch size 1"):
                model(inputs_embeds=torch.zeros(2, 1, 32), past_key_values=cache, use_cache=True)
            assert model.config._attn_implementation == "sdpa"
        _clean(cls)
        # a sliding-window layer at or after dycoke_l - 1
        _install()
        from transformers import Qwen2Config
        torch.manual_seed(0)
        model = _qwen2_cls()(Qwen2Config(vocab_size=64, hidden_size=32, intermediate_size=64, num_hidden_layers=3, num_attention_heads=4,
                                         num_key_value_heads=2, max_position_embeddings=8192, attn_implementation="sdpa",
                                         use_sliding_window=True, sliding_window=4096,
                                         layer_types=["full_attention", "full_attention", "sliding_attention"])).eval()
        with pytest.raises(NotImplementedError, match="sliding-window"):
            _decode_once(model)
        _clean(cls)
        # with the library's own kernels installed the forward refuses head dims and dtypes they do not take, before any launch
        MPI.replace_qwen2_with_dycoke_attn(sa_prune_ratio=PRUNE, dycoke_l=2)
        cls.sttm_dycoke_fn = staticmethod(dycoke_oracle.dycoke_ttm)
        with pytest.raises(NotImplementedError, match="head dimension 8"):
            _decode_once(qwen2_model(layers=3))
        with pytest.raises(NotImplementedError, match="float64"):
            _decode_once(qwen2_model(C=256, layers=3).double(), x=torch.zeros(1, 1, 256, dtype=torch.float64))
    finally:
        _clean(cls)


def test_wrapper_refusals():
    from sttm_amd import dycoke_decode as DD
    q, k = torch.zeros(1, 4, 1, 64), torch.zeros(1, 2, 9, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DD.decode_attn_scores(q, k, 0.125)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DD.gathered_decode_attention(q, k, k, torch.arange(3, dtype=torch.int32), 0.125)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DD.select_keep(torch.zeros(9), 1, 5, 2)
    with pytest.raises(RuntimeError, match="out of range"):
        DD.keep_geometry(20, 3, 54, 18)
    assert DD.keep_geometry(70, 3, 54, 10) == (54, 13, 26)
    assert DD.num_keep_of(25088, 0.8) == R.num_keep_of(25088, 0.8) == 5017


def test_c_abi_refusals():
    """Host-side validation of the entry points (nothing is launched: every call fails before it reaches a kernel)."""
    lib = _lib.load()
    assert lib.sttm_decode_workspace_bytes(28, 12200, 5100) >= 28 * 12200 * 4
    assert lib.sttm_decode_workspace_bytes(300, 100, 10) == 0 and "query heads" in _lib.last_error()
    assert lib.sttm_decode_workspace_bytes(4, 100, 101) == 0
    assert lib.sttm_decode_workspace_bytes(0, 100, 10) == 0
    buf = torch.zeros(4096, dtype=torch.float32)
    ptr = buf.data_ptr()
    ptr += (-ptr) % 16
    sc = lambda D, dtype=_lib.STTM_F32, Hq=4, Hkv=2, ws=4096: lib.sttm_decode_attn_scores(    # noqa: E731
        ptr, D, ptr, 8 * D, D, Hq, Hkv, 8, D, dtype, 0.1, ptr, ws, ptr, None)
    assert sc(32) == _lib.ERR_UNSUPPORTED and "head dimension 32" in _lib.last_error()
    assert sc(64, dtype=5) == _lib.ERR_ARG
    assert sc(64, Hq=3) == _lib.ERR_ARG
    assert sc(64, ws=16) == _lib.ERR_ARG and "workspace" in _lib.last_error()
    assert lib.sttm_decode_attn_scores(ptr + 4, 64, ptr, 512, 64, 4, 2, 8, 64, 0, 0.1, ptr, 4096, ptr, None) == _lib.ERR_UNSUPPORTED
    assert "16-byte" in _lib.last_error()
    assert lib.sttm_decode_select_keep(ptr, 40, 3, 54, 48, ptr, 51, None) == _lib.ERR_ARG and "out of range" in _lib.last_error()
    assert lib.sttm_decode_select_keep(ptr, 40, 3, 54, 10, ptr, 12, None) == _lib.ERR_ARG and "n_keep" in _lib.last_error()
    assert lib.sttm_decode_attn_gathered(ptr, 64, ptr, 512, 64, ptr, 512, 64, 4, 2, 8, 64, 0, 0.1, ptr, 0, ptr, 4096, ptr, None) == _lib.ERR_ARG


def test_dispatcher_still_refuses_the_name_and_points_at_the_installer():
    with pytest.raises(NotImplementedError, match="replace_qwen2_with_dycoke_attn"):
        MPI.replace_qwen2_by_sparse_attn("dycoke")


def test_restore_leaves_nothing_behind():
    from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS
    cls = _qwen2_cls()
    original = cls.forward
    before = set(cls.__dict__)
    try:
        MPI.replace_qwen2_with_dycoke_attn()
        assert cls.forward is MPI._qwen2_forward_with_merge and MPI.DYCOKE_ATTN in ALL_ATTENTION_FUNCTIONS
        assert cls.dycoke_l == 3 and cls.dycoke_p == 0.8 and cls.sa_prune_ratio == 0.7 and cls.sa_start_layer_idx == 0     # :452
    finally:
        MPI.restore_qwen2()
    assert cls.forward is original and MPI.DYCOKE_ATTN not in ALL_ATTENTION_FUNCTIONS
    left = set(cls.__dict__) - before
    assert not {n for n in left if "dycoke_l" in n or "dycoke_p" in n or "decode" in n or n == "_sttm_original_forward"}, left
    if "sttm_dycoke_fn" in cls.__dict__:
        del cls.sttm_dycoke_fn


NEW_SYMBOLS = ("sttm_decode_workspace_bytes", "sttm_decode_attn_scores", "sttm_decode_select_keep", "sttm_decode_attn_gathered")


def test_header_binding_and_library_agree_on_the_new_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sttm_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        decl = re.search(rf"\b{name}\s*\(([^;]*)\)\s*;", text)
        assert decl, f"{name} is not declared in include/sttm_hip.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == decl.group(1).count(",") + 1, name
    assert lib.sttm_abi_version() == _lib.ABI_VERSION == 8
    assert "dycoke_decode.hip" in __import__("sttm_amd.build", fromlist=["SOURCES"]).SOURCES


def test_decode_kernels_use_no_scratch():
    from tests.test_kernel_resources import _kernels_of
    lib = os.path.join(REPO, "sttm_amd", "lib", "libsttm_hip.so")
    found = {n: v for n, v in _kernels_of(lib).items() if "k_dec_" in n}
    for frag, count in (("k_dec_logits", 6), ("k_dec_gathered", 6), ("k_dec_combine", 6), ("k_dec_score", 1), ("k_dec_select", 1)):
        names = [n for n in found if frag in n]
        assert len(names) == count, (frag, names)
    for name, (priv, _) in found.items():
        assert priv == 0, f"{name}: private_segment_fixed_size = {priv}"
