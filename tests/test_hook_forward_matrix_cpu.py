"""The patched decoder forward, one (model class x pattern) cell at a time, without a GPU: the oracle restatements are injected as
`sttm_*_fn` and every expected value comes from running the UNPATCHED decoder layers by hand around the `patch_hooks` function.

Cells that other files already pin at forward level: Qwen2 x quadtree, Qwen2-VL x quadtree, Qwen2 x pyrd, Qwen2 x quadtree-abl-pos
(test_patch_glue.py); both classes x quadtree on batches (test_batched_hook_cpu.py); Qwen2 x dycoke (test_dycoke_decode_cpu.py); both
classes x tome with a snippet size (test_tome_snippet_cpu.py).  This file adds the rest, and one test per place where the two model
families differ on purpose (or by accident that callers may rely on): what is returned as the cache, how many layers run, what the
layers receive as `position_ids`, which state is reset at prefill, what an unknown pattern name does, and who gets `head_dim`."""
import contextlib

import pytest
import torch

from oracle import dycoke_oracle, octree_oracle
from oracle import sttm_oracle as O
from sttm_amd import monkey_patch_interface as MPI
from sttm_amd import patch_hooks
from tests._batched_common import (THRESH, left_pad, mrope_ids, positions_1d, prompt_rows, qwen2_model, qwen2vl_model, set_one,
                                   set_rows)
from tests._pack_ref import pack_merged_batch_ref

pytest.importorskip("transformers")

SPEC = (5, 4, 8, 8, 7)               # n_sys, T, H, W, n_inst: T = 4 frames of 8 x 8
SPEC_DYCOKE = (5, 6, 4, 4, 7)        # the DyCoke oracle needs T >= 5
SPEC_OCTREE = (5, 5, 4, 4, 7)        # one 4 x 4 x 4 cube and a remainder frame
QT = (THRESH["sa_tree_thresh"], THRESH["sa_tree_temporal_thresh"], THRESH["sa_tree_root_level"], False)
_INJECTED = ("sttm_merge_fn", "sttm_merge_batch_fn", "sttm_pack_fn", "sttm_tome_fn", "sttm_tome_snippet_fn", "sttm_dycoke_fn",
             "sttm_octree_fn", "sttm_resize_fn", "sa_tome_snippet_size")


def _qwen2_cls():
    from transformers.models.qwen2.modeling_qwen2 import Qwen2Model
    return Qwen2Model


def _qwen2vl_cls():
    from transformers.models.qwen2_vl.modeling_qwen2_vl import Qwen2VLTextModel
    return Qwen2VLTextModel


def _cls(vl):
    return _qwen2vl_cls() if vl else _qwen2_cls()


def _model(vl, **kw):
    return qwen2vl_model(**kw) if vl else qwen2_model(**kw)


@contextlib.contextmanager
def patched(install, vl=False, **fns):
    """install() with the given functions bound on the class (an installer fills only what is absent); all undone on exit."""
    cls = _cls(vl)
    try:
        for name, fn in fns.items():
            setattr(cls, name, staticmethod(fn))
        install()
        yield cls
    finally:
        MPI.restore_qwen2()
        for c in (_qwen2_cls(), _qwen2vl_cls()):
            for name in _INJECTED:
                if name in c.__dict__:
                    delattr(c, name)


def oracle_batch(videos, *args, **kw):
    return [O.get_quadtree_features(v, *args, **kw) for v in videos]


def _prompt(spec, C=32):
    hs = prompt_rows([spec], C)[0].unsqueeze(0)
    return hs, spec[0], spec[1] * spec[2] * spec[3]


def _ids(vl, L):
    return mrope_ids(L)[:, None] if vl else torch.arange(L)[None]


def _by_hand(model, hs, pos, hook, at=1, n_layers=None, layer_ids=lambda p: p):
    """The unpatched layers run one after the other; hook(h, pos) -> (h, pos) before layer `at`."""
    h = hs
    pe = model.rotary_emb(h, pos)
    for i, layer in enumerate(model.layers[:n_layers]):
        if i == at:
            h, pos = hook(h, pos)
            pe = model.rotary_emb(h, pos)
        h = layer(h, attention_mask=None, position_embeddings=pe, position_ids=layer_ids(pos))
    return model.norm(h)


def _no_ids(_pos):
    return None                      # a Qwen2-VL layer receives the text ids, which 3-row mRoPE ids do not have


def _quadtree_hook(vl, spec):
    start, T, H, W = spec[0], spec[1], spec[2], spec[3]
    if vl:
        return lambda h, p: patch_hooks.quadtree_merge_qwen2vl(h, p, start, T * H * W, T, H, W, O.get_quadtree_features, *QT)[:2]
    return lambda h, p: patch_hooks.quadtree_merge_llava(h, p, start, T * H * W, T, O.get_quadtree_features, *QT)[:2]


def _install_quadtree(vl, **kw):
    fn = MPI.replace_qwen2vl_with_quadtree_attn if vl else MPI.replace_qwen2_with_quadtree_attn
    return lambda: fn(sa_start_layer_idx=1, **{**THRESH, **kw})


def _tome_hook(vl, spec, ratio=0.5):
    start, T, H, W = spec[0], spec[1], spec[2], spec[3]
    kw = dict(H=H, W=W, gather_positions=True) if vl else {}
    return lambda h, p: patch_hooks.tome_merge(h, p, start, T * H * W, T, O.get_tome_features, ratio, "video", **kw)[:2]


def _install_tome(vl, **kw):
    fn = MPI.replace_qwen2vl_with_tome_attn if vl else MPI.replace_qwen2_with_tome_attn
    return lambda: fn(sa_start_layer_idx=1, sa_prune_ratio=0.5, sa_tome_ver="video", **kw)


# ---- cells ---------------------------------------------------------------------------------------------------------------------
def test_qwen2_octree_forward_matches_manual_layers_and_keeps_no_index():
    model = qwen2_model()
    hs, start, length = _prompt(SPEC_OCTREE)
    T = SPEC_OCTREE[1]
    set_one(model, SPEC_OCTREE)
    model.merged_token_1d_idx = "stale"
    with patched(lambda: MPI.replace_qwen2_by_sparse_attn("octree", sa_start_layer_idx=1, sa_tree_thresh=0.5, sa_tree_root_level=0),
                 sttm_octree_fn=octree_oracle.get_octree_features), torch.inference_mode():
        out = model(inputs_embeds=hs, use_cache=False).last_hidden_state
        ref = _by_hand(model, hs, _ids(False, hs.shape[1]),
                       lambda h, p: patch_hooks.octree_merge(h, p, start, length, T, octree_oracle.get_octree_features, 0.5, 0))
    assert model.merged_token_1d_idx is None                        # the reference's octree hook keeps no token index
    assert out.shape == ref.shape and out.shape[1] < hs.shape[1]
    assert torch.allclose(out, ref, atol=1e-5)


@pytest.mark.parametrize("vl", [False, True], ids=["qwen2", "qwen2vl"])
def test_dycoke_stage1_forward_matches_manual_layers(vl):
    """Qwen2 truncates the position ids, Qwen2-VL gathers the 3-D ids of the kept tokens."""
    model = _model(vl)
    hs, start, length = _prompt(SPEC_DYCOKE)
    T, L = SPEC_DYCOKE[1], hs.shape[1]
    set_one(model, SPEC_DYCOKE, vl)
    pos = _ids(vl, L)
    seen = []

    def hook(h, p):
        h, p, idx = patch_hooks.dycoke_merge(h, p, start, length, T, dycoke_oracle.dycoke_ttm, 0.5, gather_positions=vl)
        seen.append((p, idx))
        return h, p
    with patched(lambda: MPI.replace_qwen2_by_sparse_attn("dycoke-stage1", sa_start_layer_idx=1, sa_prune_ratio=0.5), vl,
                 sttm_dycoke_fn=dycoke_oracle.dycoke_ttm) as cls, torch.inference_mode():
        assert cls.sttm_pattern == "dycoke-stage1"
        out = model(inputs_embeds=hs, position_ids=pos, use_cache=False).last_hidden_state
        ref = _by_hand(model, hs, pos, hook, layer_ids=_no_ids if vl else (lambda p: p))
    p2, idx = seen[0]
    n = idx.numel()
    assert torch.equal(model.merged_token_1d_idx, idx) and 0 < n < length
    if vl:      # system ids ++ visual ids gathered by the kept-token index ++ instruction ids
        end = start + length
        assert torch.equal(p2, torch.cat([pos[:, :, :start], pos[:, :, start:end][:, :, idx], pos[:, :, end:]], dim=-1))
        assert not torch.equal(p2, pos[:, :, :p2.shape[-1]])
    else:
        assert torch.equal(p2, pos[:, :L - length + n])
    assert out.shape == ref.shape == (1, L - length + n, 32)
    assert torch.allclose(out, ref, atol=1e-5)


@pytest.mark.parametrize("vl", [False, True], ids=["qwen2", "qwen2vl"])
def test_tome_forward_without_snippet_size_matches_manual_layers(vl):
    """sa_tome_snippet_size=None: `sttm_tome_fn(video, prune_ratio, tome_ver)` as the reference dispatches it."""
    model = _model(vl)
    hs, _, length = _prompt(SPEC)
    set_one(model, SPEC, vl)
    pos = _ids(vl, hs.shape[1])
    calls = []

    def tome(video, ratio, ver):
        calls.append((tuple(video.shape), ratio, ver))
        return O.get_tome_features(video, ratio, ver)
    with patched(_install_tome(vl), vl, sttm_tome_fn=tome) as cls, torch.inference_mode():
        assert cls.sa_tome_snippet_size is None and cls.sttm_pattern == "tome"
        out = model(inputs_embeds=hs, position_ids=pos, use_cache=False).last_hidden_state
        idx = model.merged_token_1d_idx
        ref = _by_hand(model, hs, pos, _tome_hook(vl, SPEC), layer_ids=_no_ids if vl else (lambda p: p))
    assert calls == [((4, 32, 8, 8), 0.5, "video")]
    assert idx.dtype == torch.int64 and idx.numel() == length // 2
    assert out.shape == ref.shape == (1, hs.shape[1] - length // 2, 32)
    assert torch.allclose(out, ref, atol=1e-5)


# ---- where the two families differ ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vl", [False, True], ids=["qwen2", "qwen2vl"])
def test_cache_return(vl):
    """use_cache=False: Qwen2 returns no cache, Qwen2-VL hands back the cache object it was given."""
    from transformers.cache_utils import DynamicCache
    model = _model(vl)
    hs, _, _ = _prompt(SPEC)
    set_one(model, SPEC, vl)
    with patched(_install_quadtree(vl), vl, sttm_merge_fn=O.get_quadtree_features), torch.inference_mode():
        assert model(inputs_embeds=hs, use_cache=False).past_key_values is None
        cache = DynamicCache(config=model.config)
        res = model(inputs_embeds=hs, past_key_values=cache, use_cache=False)
        assert res.past_key_values is (cache if vl else None)
        assert isinstance(model(inputs_embeds=hs, use_cache=True).past_key_values, DynamicCache)
        cache = DynamicCache(config=model.config)
        assert model(inputs_embeds=hs, past_key_values=cache, use_cache=True).past_key_values is cache


@pytest.mark.parametrize("vl", [False, True], ids=["qwen2", "qwen2vl"])
def test_layer_count(vl):
    """config.num_hidden_layers below len(model.layers): Qwen2 runs only the first num_hidden_layers layers, Qwen2-VL runs all."""
    model = _model(vl)
    model.config.num_hidden_layers = 2
    assert len(model.layers) == 3
    hs, _, _ = _prompt(SPEC)
    set_one(model, SPEC, vl)
    pos = _ids(vl, hs.shape[1])
    ran = []
    handles = [layer.register_forward_pre_hook(lambda m, a, i=i: ran.append(i)) for i, layer in enumerate(model.layers)]
    try:
        with patched(_install_quadtree(vl), vl, sttm_merge_fn=O.get_quadtree_features), torch.inference_mode():
            out = model(inputs_embeds=hs, position_ids=pos, use_cache=False).last_hidden_state
            assert ran == ([0, 1, 2] if vl else [0, 1])
            ref = _by_hand(model, hs, pos, _quadtree_hook(vl, SPEC), n_layers=None if vl else 2,
                           layer_ids=_no_ids if vl else (lambda p: p))
    finally:
        for h in handles:
            h.remove()
    assert out.shape == ref.shape and out.shape[1] < hs.shape[1]
    assert torch.allclose(out, ref, atol=1e-5)


def _capture_layer_kwargs(model, store):
    return [layer.register_forward_pre_hook(lambda m, a, kw, i=i: store.append((i, dict(kw))), with_kwargs=True)
            for i, layer in enumerate(model.layers)]


@pytest.mark.parametrize("pattern", ["quadtree", "tome"])
def test_qwen2vl_four_row_position_ids(pattern):
    """[4, B, L] ids = the text row plus three mRoPE rows: the rotary embedding comes from the three GATHERED rows, the layers receive
    the text row, truncated to the new length after the merge."""
    model = qwen2vl_model()
    hs, _, _ = _prompt(SPEC)
    L = hs.shape[1]
    set_one(model, SPEC, True)
    text = 100 + torch.arange(L)[None]           # consecutive: ids that jump would be read as packed sequences
    pos4 = torch.cat([text[None], _ids(True, L)])
    install, hook, fns = {"quadtree": (_install_quadtree(True), _quadtree_hook(True, SPEC), dict(sttm_merge_fn=O.get_quadtree_features)),
                          "tome": (_install_tome(True), _tome_hook(True, SPEC), dict(sttm_tome_fn=O.get_tome_features))}[pattern]
    seen, gathered = [], []
    with patched(install, True, **fns), torch.inference_mode():
        handles = _capture_layer_kwargs(model, seen)
        try:
            out = model(inputs_embeds=hs, position_ids=pos4, use_cache=False).last_hidden_state
        finally:
            for h in handles:
                h.remove()
        ref = _by_hand(model, hs, pos4[1:], lambda h, p: gathered.append(hook(h, p)) or gathered[0], layer_ids=_no_ids)
    n = out.shape[1]
    assert n < L and [i for i, _ in seen] == [0, 1, 2]
    assert torch.equal(seen[0][1]["position_ids"], text)
    for _, kw in seen[1:]:
        assert torch.equal(kw["position_ids"], text[..., :n])
    # the embeddings every later layer received are those of the gathered three rows
    for want, got in zip(model.rotary_emb(*gathered[0]), seen[1][1]["position_embeddings"]):
        assert torch.equal(want, got)
    assert torch.allclose(out, ref, atol=1e-5)


def test_qwen2vl_four_row_position_ids_on_a_batch():
    """The batched hook keeps the text row per prompt: row b's valid columns keep its first L'_b text ids, pads get 1."""
    specs = [(5, 4, 8, 8, 7), (0, 3, 8, 8, 2)]
    model = qwen2vl_model()
    rows = prompt_rows(specs, 32, seed=11)
    hs, mask = left_pad(rows, extra_pad=(2,))
    B, L = mask.shape
    lengths = [r.shape[0] for r in rows]
    pos3 = torch.ones(3, B, L, dtype=torch.long)
    for b, n in enumerate(lengths):
        pos3[:, b, L - n:] = mrope_ids(n)
    text = 100 + positions_1d(mask)
    seen = []
    handles = _capture_layer_kwargs(model, seen)
    try:
        with patched(_install_quadtree(True), True, sttm_merge_fn=O.get_quadtree_features, sttm_merge_batch_fn=oracle_batch,
                     sttm_pack_fn=pack_merged_batch_ref), torch.inference_mode():
            set_rows(model, specs, True)
            out = model(inputs_embeds=hs, attention_mask=mask, position_ids=torch.cat([text[None], pos3]), use_cache=False).last_hidden_state
    finally:
        for h in handles:
            h.remove()
    Lout = out.shape[1]
    assert torch.equal(seen[0][1]["position_ids"], text)
    got = seen[1][1]["position_ids"]
    assert got.shape == (B, Lout) and torch.equal(got, seen[2][1]["position_ids"])
    for b, n in enumerate(lengths):
        kept = lengths[b] - specs[b][1] * 64 + model.merged_token_1d_idx[b].numel()
        assert torch.equal(got[b, Lout - kept:], text[b, L - n:L - n + kept])
        assert torch.equal(got[b, :Lout - kept], torch.ones(Lout - kept, dtype=got.dtype))


@pytest.mark.parametrize("vl", [False, True], ids=["qwen2", "qwen2vl"])
def test_unknown_pattern_takes_the_tome_hook(vl):
    model = _model(vl)
    hs, _, length = _prompt(SPEC)
    set_one(model, SPEC, vl)
    pos = _ids(vl, hs.shape[1])
    with patched(_install_tome(vl), vl, sttm_tome_fn=O.get_tome_features) as cls, torch.inference_mode():
        try:
            cls.sttm_pattern = "no-such-pattern"
            out = model(inputs_embeds=hs, position_ids=pos, use_cache=False).last_hidden_state
        finally:
            cls.sttm_pattern = "tome"
        ref = _by_hand(model, hs, pos, _tome_hook(vl, SPEC), layer_ids=_no_ids if vl else (lambda p: p))
    assert out.shape[1] == hs.shape[1] - length // 2 and torch.allclose(out, ref, atol=1e-5)


def _recording_merge(calls):
    def fn(video, *args, **kw):
        calls.append(dict(kw))
        return O.get_quadtree_features(video, *args, **kw)
    return fn


def test_qwen2vl_quadtree_runs_without_sim_per_head():
    """The Qwen2-VL installer sets no `sim_per_head`, and its merge function is never handed a `head_dim`."""
    cls = _qwen2vl_cls()
    model = qwen2vl_model()
    hs, _, _ = _prompt(SPEC)
    calls, bcalls = [], []

    def batch(videos, *args, **kw):
        bcalls.append(dict(kw))
        return oracle_batch(videos, *args, **kw)
    with patched(_install_quadtree(True), True, sttm_merge_fn=_recording_merge(calls), sttm_merge_batch_fn=batch,
                 sttm_pack_fn=pack_merged_batch_ref), torch.inference_mode():
        assert not hasattr(cls, "sim_per_head")
        set_one(model, SPEC, True)
        out = model(inputs_embeds=hs, use_cache=False).last_hidden_state
        set_rows(model, [SPEC], True)
        out_b = model(inputs_embeds=hs, attention_mask=torch.ones(1, hs.shape[1], dtype=torch.long), use_cache=False).last_hidden_state
    assert calls == [dict(slow_ver=False)] and bcalls == [dict(slow_ver=False)]
    assert out.shape[1] < hs.shape[1] and out_b.shape == out.shape


@pytest.mark.parametrize("sim_per_head", [False, True])
def test_qwen2_hands_head_dim_to_the_merge_only_with_sim_per_head(sim_per_head):
    model = qwen2_model()
    hs, _, _ = _prompt(SPEC)
    want = dict(slow_ver=False, head_dim=model.layers[1].self_attn.head_dim if sim_per_head else None)
    assert model.layers[1].self_attn.head_dim == 8
    calls, bcalls = [], []

    def batch(videos, *args, **kw):
        bcalls.append(dict(kw))
        return oracle_batch(videos, *args, **kw)
    with patched(_install_quadtree(False, sim_per_head=sim_per_head), sttm_merge_fn=_recording_merge(calls), sttm_merge_batch_fn=batch,
                 sttm_pack_fn=pack_merged_batch_ref), torch.inference_mode():
        set_one(model, SPEC)
        model(inputs_embeds=hs, use_cache=False)
        set_rows(model, [SPEC])
        model(inputs_embeds=hs, attention_mask=torch.ones(1, hs.shape[1], dtype=torch.long), use_cache=False)
    assert calls == [want] and bcalls == [want]
    calls.clear()
    with patched(lambda: MPI.replace_qwen2_by_sparse_attn("quadtree-abl-pos", sa_start_layer_idx=1, sim_per_head=sim_per_head, **THRESH),
                 sttm_merge_fn=_recording_merge(calls)), torch.inference_mode():
        set_one(model, SPEC)
        model(inputs_embeds=hs, use_cache=False)
    assert calls == [dict(want, pos_embs=None, pos_emb_weighted_avg=False)]


@pytest.mark.parametrize("vl", [False, True], ids=["qwen2", "qwen2vl"])
def test_prefill_resets_the_cache_state_of_its_family(vl):
    """Both families drop a batched merge's key mask at prefill; only Qwen2 has (and resets) DyCoke decode state."""
    from transformers.cache_utils import DynamicCache
    model = _model(vl)
    hs, _, _ = _prompt(SPEC)
    set_one(model, SPEC, vl)
    with patched(_install_quadtree(vl), vl, sttm_merge_fn=O.get_quadtree_features), torch.inference_mode():
        cache = DynamicCache(config=model.config)
        cache.sttm_merged_mask = (torch.ones(1, 3), 3)
        cache.sttm_dycoke = (1, 2)
        model(inputs_embeds=hs, past_key_values=cache, use_cache=True)
    assert cache.sttm_merged_mask is None
    assert cache.sttm_dycoke == ((1, 2) if vl else None)


@pytest.mark.parametrize("vl", [False, True], ids=["qwen2", "qwen2vl"])
def test_hook_stays_out_without_video_attributes_and_at_decode(vl):
    """No `image_token_length` on the module: the patched forward is the installed one.  A decode step never merges."""
    model = _model(vl)
    hs, _, _ = _prompt(SPEC)
    calls = []
    with torch.inference_mode():
        plain = model(inputs_embeds=hs, use_cache=False).last_hidden_state
        with patched(_install_quadtree(vl), vl, sttm_merge_fn=_recording_merge(calls)):
            out = model(inputs_embeds=hs, use_cache=False).last_hidden_state
            assert not calls and torch.equal(out, plain)
            set_one(model, SPEC, vl)
            res = model(inputs_embeds=hs, use_cache=True)
            assert len(calls) == 1
            step = model(inputs_embeds=hs[:, :1], past_key_values=res.past_key_values, use_cache=True).last_hidden_state
            assert len(calls) == 1 and step.shape == (1, 1, 32)
