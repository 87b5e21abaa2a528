"""L2 installer with the reference's names and keyword arguments (token_merging_utils/monkey_patch_interface.py:17-38).

`replace_qwen2_by_sparse_attn(pattern_name, **kwargs)` dispatches on the same pattern names.  "quadtree" and "tome" --
the two patterns on the hot path -- and the baselines that share their hook ("quadtree-abl-pos", "pyrd", "dycoke-stage1",
"octree") are implemented: like the reference they store their configuration as CLASS attributes on the decoder model
class and overwrite its `.forward` (quadtree_attn_monkey_patch.py:177-187, tome_attn_monkey_patch.py:163-171).  Full DyCoke
(stage 1 + decode-time KV selection) is installed by `replace_qwen2_with_dycoke_attn`; the dispatcher still refuses the name
"dycoke" and points there.  Only the FrameFusion baselines and the plotting variants raise NotImplementedError, with a message
that says so.

The reference pins transformers==4.45.2 and patches a verbatim copy of that version's Qwen2Model.forward.  This
build targets the transformers that is installed (5.x decoder-layer API): `_forward` below is the installed decoder forward
with the merge step inserted before layer `sa_start_layer_idx` on prefill.  It is ONE skeleton for both model families; what
differs between Qwen2 and the Qwen2-VL text model is the `_Family` record it is called with (`_QWEN2`, `_QWEN2VL`): position-id
handling, the batched hook, the layer slice, what is returned as the cache, and the table `pattern -> (fires, hook)` of the
batch-1 hooks.  Every `replace_*` goes through the one `_install`.
State read by the hook is the same as the reference's: `self.image_token_start_index`, `self.image_token_length`, `self.num_frame`
(0-d tensors set by generate(), llava/model/language_model/llava_qwen.py:141-143), plus `image_H/image_W` for Qwen2-VL.
For "quadtree" they may also be 1-D tensors of length B: the batched hook of a left-padded batch ("Batched prompts").
"""
import importlib
from collections import namedtuple

import torch

from . import patch_hooks
from .quadtree_interface import (get_quadtree_features, get_quadtree_features_batch_reused, get_quadtree_features_into,
                                 pack_merged_batch)
from .tome_interface import get_tome_features, get_tome_features_snippet

_UNIMPLEMENTED = {
    "quadtree_vis": "visualisation variant",
}


def _item(v):
    return int(v.item()) if torch.is_tensor(v) else int(v)


def _is_prefill(past_key_values):
    return past_key_values is None or past_key_values.get_seq_length() == 0


def _rebuild_masks(self, mask_map, hidden_states):
    """Masks for the SHORTER sequence after the merge.  The reference computes `causal_mask` once before the layer loop
    and never updates it (quadtree_attn_monkey_patch.py:60-66 vs :88-117), which only works when that mask is None
    (flash-attention / SDPA without padding).  Here the masks are rebuilt on the merged hidden states, so eager attention
    stays causal and sliding-window layers keep their window; for SDPA / flash this returns None exactly like before."""
    from transformers.masking_utils import create_causal_mask, create_sliding_window_causal_mask
    # prefill: the layers from here on see an empty cache, so keys = the merged sequence itself (no past offset: the
    # cache object already holds the LONG sequence of the earlier layers and must not be consulted); no position ids
    # either -- gathered (non-monotonic) ids would be mistaken for packed sequences
    mk = dict(config=self.config, inputs_embeds=hidden_states, attention_mask=None, past_key_values=None, position_ids=None)
    out = {}
    for k in mask_map:
        out[k] = create_sliding_window_causal_mask(**mk) if k == "sliding_attention" else create_causal_mask(**mk)
    return out


# ---- batched prompts ("quadtree" on B > 1 left-padded rows) ---------------------------------------------------------------
_QWEN2_ROW_ATTRS = ("image_token_start_index", "image_token_length", "num_frame")
_QWEN2VL_ROW_ATTRS = _QWEN2_ROW_ATTRS + ("image_H", "image_W")


def _per_row(v, B, name):
    """A hook attribute as B ints: a 0-d tensor or an int is the same for every row, a 1-D tensor has one entry per row."""
    if torch.is_tensor(v) and v.dim() == 1:
        if v.numel() != B:
            raise ValueError(f"{name} has {v.numel()} entries for a batch of {B} prompts")
        return [int(x) for x in v.tolist()]
    return [_item(v)] * B


def _batched_rows(self, inputs_embeds, attention_mask, prefilling, names):
    """None (the batch-1 hook) or (pads, per-row attribute lists) when the batched quadtree hook runs on this prefill: B > 1 or an
    attribute is 1-D.  Pad counts come from the 2-D attention mask, read once before any layer is enqueued."""
    if not prefilling or self.sttm_pattern != "quadtree" or getattr(self, "image_token_length", None) is None:
        return None
    B, L = inputs_embeds.shape[:2]
    if B == 1 and not any(torch.is_tensor(getattr(self, n, None)) and getattr(self, n).dim() == 1 for n in names):
        return None
    attrs = [_per_row(getattr(self, n), B, n) for n in names]
    if attention_mask is None:
        return [0] * B, attrs
    if not torch.is_tensor(attention_mask) or attention_mask.dim() != 2 or tuple(attention_mask.shape) != (B, L):
        raise ValueError("the batched quadtree hook needs the 2-D [B, L] attention mask of the prompts")
    m = attention_mask.to(torch.bool)
    valid, first = torch.stack([m.sum(-1), m.to(torch.int32).argmax(-1)]).tolist()
    pads = [L - v for v in valid]
    if any(v == 0 or f != p for v, f, p in zip(valid, first, pads)):
        raise ValueError("the batched quadtree hook needs LEFT-padded prompts (generate reads the last column)")
    return pads, attrs


def _positions_from_mask(attention_mask, inputs_embeds):
    """What generate passes for a left-padded batch: every row counts from its first valid token, pads get 1."""
    B, L = inputs_embeds.shape[:2]
    if attention_mask is None:
        return torch.arange(L, device=inputs_embeds.device).unsqueeze(0).expand(B, -1)
    m = attention_mask.to(device=inputs_embeds.device, dtype=torch.long)
    return (m.cumsum(-1) - 1).masked_fill(m == 0, 1)


def _merged_layout_masks(self, mask_map, hidden_states, mask2d, past_key_values):
    """Masks of the layers from sa_start_layer_idx on, over the merged layout's 2-D key mask.  Prefill (past_key_values None): the
    keys are the merged block itself.  Decode: sized against the first such layer of each type in the cache (the earlier layers
    hold the long layout)."""
    from transformers.masking_utils import create_causal_mask, create_sliding_window_causal_mask
    types = self.config.layer_types
    out = {}
    for k in mask_map:
        kw = dict(config=self.config, inputs_embeds=hidden_states, attention_mask=mask2d, past_key_values=past_key_values,
                  position_ids=None)
        if past_key_values is not None:
            first = next((i for i in range(self.sa_start_layer_idx, len(types)) if types[i] == k), None)
            if first is None:
                out[k] = mask_map[k]
                continue
            kw["layer_idx"] = first
        out[k] = create_sliding_window_causal_mask(**kw) if k == "sliding_attention" else create_causal_mask(**kw)
    return out


def _decode_masks(self, mask_map, inputs_embeds, attention_mask, past_key_values):
    """Decode step after a batched merge: the merged layout's prefill key mask (kept with the cache) extended by the columns generate
    appended after the prompt, one valid column per generated token.  None when the cache holds no batched merge."""
    state = getattr(past_key_values, "sttm_merged_mask", None) if past_key_values is not None else None
    if state is None:
        return None
    m0, L0 = state
    total = past_key_values.get_seq_length(self.sa_start_layer_idx) + inputs_embeds.shape[1]
    extra = total - m0.shape[1]
    if torch.is_tensor(attention_mask) and attention_mask.dim() == 2 and attention_mask.shape[1] == L0 + extra:
        tail = attention_mask[:, L0:].to(device=m0.device, dtype=m0.dtype)
    else:
        tail = m0.new_ones((m0.shape[0], extra))
    return _merged_layout_masks(self, mask_map, inputs_embeds, torch.cat([m0, tail], dim=1), past_key_values)


def _truncate_rows(ids, pads, mask2d, L):
    """[B or 1, L] ids -> [B, L'max]: row b's valid columns keep its first L'_b ids (the batch-1 truncation), pads get 1."""
    B, Lout = mask2d.shape
    ids = ids.expand(B, L)
    shift = torch.tensor([Lout - int(v) - p for v, p in zip(mask2d.sum(-1).tolist(), pads)], device=ids.device)
    col = (torch.arange(Lout, device=ids.device)[None] - shift[:, None]).clamp(0, L - 1)
    return torch.where(mask2d.to(torch.bool), ids.gather(1, col), torch.ones_like(col))


def _keep_merged_mask(past_key_values, mask2d, L):
    if past_key_values is not None:
        past_key_values.sttm_merged_mask = (mask2d, L)


def _reset_merged_mask(past_key_values):
    if past_key_values is not None and getattr(past_key_values, "sttm_merged_mask", None) is not None:
        past_key_values.sttm_merged_mask = None


# ---- DyCoke stage 2 ("dycoke": decode-time KV selection, dycoke_attn_monkey_patch.py) -----------------------------------------
DYCOKE_ATTN = "sttm_dycoke"           # name of the dispatching attention function in transformers' AttentionInterface
_DECODE_FNS = ("sttm_decode_scores_fn", "sttm_decode_select_fn", "sttm_decode_attn_fn")
_DECODE_DEFAULTS = dict(zip(_DECODE_FNS, ((".dycoke_decode", fn) for fn in ("decode_attn_scores", "select_keep", "gathered_decode_attention"))))


def _resolve(default):
    """An injection default: a function, or a (module, name) pair that is imported only when it is needed."""
    if isinstance(default, tuple):
        return getattr(importlib.import_module(default[0], __package__), default[1])
    return default


class _DycokeStep:
    """State of ONE decode forward: what the dispatching attention function reads and the keep list it leaves for the later layers."""
    def __init__(self, cls, base_impl, l, start, n0, num_keep):
        self.base_impl, self.l, self.start, self.n0, self.num_keep = base_impl, l, start, n0, num_keep
        self.scores_fn, self.select_fn, self.attn_fn = cls.sttm_decode_scores_fn, cls.sttm_decode_select_fn, cls.sttm_decode_attn_fn
        self.score = self.keep = None


def _dycoke_attention(module, query, key, value, attention_mask, scaling=None, **kwargs):
    """Attention function of a "dycoke" decode forward.  Layer l - 1 also yields the head-mean softmax row and the keep list (:80,
    :62-77); layers >= l attend to the kept rows of the cache (:54-60); everything else is the implementation the user configured."""
    from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS
    from transformers.models.qwen2.modeling_qwen2 import eager_attention_forward
    st = getattr(module.config, "_sttm_dycoke_step", None)
    if st is None:
        raise RuntimeError(f"the {DYCOKE_ATTN!r} attention function only runs inside a DyCoke decode forward "
                           "(replace_qwen2_with_dycoke_attn); it is not an attn_implementation of its own")
    scaling = module.scaling if scaling is None else scaling
    i = module.layer_idx
    if i >= st.l:
        return st.attn_fn(query, key, value, st.keep, scaling), None
    if i == st.l - 1:
        st.score = st.scores_fn(query, key, scaling)
        st.keep = st.select_fn(st.score, st.start, st.n0, st.num_keep)
    base = ALL_ATTENTION_FUNCTIONS.get_interface(st.base_impl, eager_attention_forward)
    return base(module, query, key, value, attention_mask, scaling=scaling, **kwargs)


def _dycoke_step(self, inputs_embeds, past_key_values):
    """None, or the _DycokeStep of this decode forward (refusals first, all before any layer runs)."""
    state = getattr(past_key_values, "sttm_dycoke", None) if past_key_values is not None else None
    if state is None or inputs_embeds.shape[1] != 1:                    # :407 `position_ids.shape[1] == 1`
        return None
    cfg, l = self.config, self.dycoke_l
    if inputs_embeds.shape[0] != 1:
        raise NotImplementedError(f"DyCoke stage 2 reads row 0 of the attention matrix (`[0, -1]`): batch size 1 only, got {inputs_embeds.shape[0]}")
    if not 1 <= l < cfg.num_hidden_layers:
        raise ValueError(f"dycoke_l = {l} must be in [1, num_hidden_layers = {cfg.num_hidden_layers}): layer dycoke_l - 1 supplies the scores")
    if self.sa_start_layer_idx > l - 1:
        raise ValueError(f"sa_start_layer_idx = {self.sa_start_layer_idx} must not exceed dycoke_l - 1 = {l - 1}: the keep list of layer "
                         "dycoke_l - 1 indexes the cache of the later layers, which must hold the same (merged) sequence")
    if any(t != "full_attention" for t in cfg.layer_types[l - 1:]):
        raise NotImplementedError(f"a sliding-window layer at or after dycoke_l - 1 = {l - 1} is not supported by DyCoke stage 2")
    head_dim = self.layers[l].self_attn.head_dim
    own = type(self).sttm_decode_attn_fn is _resolve(_DECODE_DEFAULTS["sttm_decode_attn_fn"])
    if own and head_dim not in (64, 128):
        raise NotImplementedError(f"head dimension {head_dim}: the decode kernels are built for 64 and 128")
    if own and inputs_embeds.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise NotImplementedError(f"dtype {inputs_embeds.dtype}: the decode kernels take float32, bfloat16 and float16")
    start, n0 = state
    num_keep = int(n0 * (1 - self.dycoke_p))                            # :66
    Lk = past_key_values.get_seq_length(l - 1) + 1
    window = min(start + n0, Lk) - start
    if num_keep > window:                                               # the reference's topk raises (:69)
        raise RuntimeError(f"selected index k out of range: num_keep = int({n0} * (1 - {self.dycoke_p})) = {num_keep} exceeds the "
                           f"window of {window} scores [{start}, {min(start + n0, Lk)})")
    return _DycokeStep(type(self), cfg._attn_implementation, l, start, n0, num_keep)


# ---- the batch-1 hooks: fn(self, layer, hidden_states, position_ids, position_embeddings, start, length, T) ----------------------
# -> (hidden_states, position_ids, position_embeddings or None = "compute them from the new ids", merged_token_1d_idx)
_KEEP_IDX = object()                  # in place of an index: leave `self.merged_token_1d_idx` as it is


def _head_dim(self, layer):
    return layer.self_attn.head_dim if getattr(self, "sim_per_head", False) else None


def _fused_merge_fn(cls):
    """Fused slice -> merge -> concat (the kernels write the merged rows into the new hidden-state buffer) is used
    whenever the merge function is the library's own; an injected `sttm_merge_fn` (tests) takes the plain path."""
    return get_quadtree_features_into if cls.sttm_merge_fn is get_quadtree_features else None


def _tome_merge_fn(cls):
    """The merge function the ToMe hook hands to patch_hooks.tome_merge: `sttm_tome_fn(video, prune_ratio, tome_ver)` as the
    reference dispatches it, or -- when the installer was given sa_tome_snippet_size -- per-snippet ToMe, which ignores tome_ver."""
    size = getattr(cls, "sa_tome_snippet_size", None)
    if size is None:
        return cls.sttm_tome_fn
    fn = cls.sttm_tome_snippet_fn
    return lambda video, prune_ratio, _tome_ver: fn(video, prune_ratio, size)


def _tree_args(self):
    return self.sa_tree_thresh, self.sa_tree_temporal_thresh, self.sa_tree_root_level, self.sa_tree_weighted_avg


def _with_new_embeddings(res):
    hidden_states, position_ids, idx = res
    return hidden_states, position_ids, None, idx


def _hook_quadtree(self, layer, hidden_states, position_ids, position_embeddings, start, length, T):
    return _with_new_embeddings(patch_hooks.quadtree_merge_llava(
        hidden_states, position_ids, start, length, T, type(self).sttm_merge_fn, *_tree_args(self), slow_ver=self.sttm_slow_ver,
        head_dim=_head_dim(self, layer), merge_into_fn=_fused_merge_fn(type(self))))


def _hook_quadtree_abl_pos(self, layer, hidden_states, position_ids, position_embeddings, start, length, T):
    return patch_hooks.quadtree_merge_abl_pos(                        # this hook decides its own position embeddings
        hidden_states, position_ids, position_embeddings, start, length, T, type(self).sttm_merge_fn, *_tree_args(self),
        self.pos_emb_ver, self.pos_emb_weighted_avg, self.rotary_emb, slow_ver=self.sttm_slow_ver, head_dim=_head_dim(self, layer))


def _hook_dycoke(self, layer, hidden_states, position_ids, position_embeddings, start, length, T):
    return _with_new_embeddings(patch_hooks.dycoke_merge(
        hidden_states, position_ids, start, length, T, type(self).sttm_dycoke_fn, self.sa_prune_ratio))


def _hook_octree(self, layer, hidden_states, position_ids, position_embeddings, start, length, T):
    hidden_states, position_ids = patch_hooks.octree_merge(
        hidden_states, position_ids, start, length, T, type(self).sttm_octree_fn, self.sa_tree_thresh, self.sa_tree_root_level)
    return hidden_states, position_ids, None, None                    # the reference's octree hook keeps no token index


def _hook_tome(self, layer, hidden_states, position_ids, position_embeddings, start, length, T):
    return _with_new_embeddings(patch_hooks.tome_merge(
        hidden_states, position_ids, start, length, T, _tome_merge_fn(type(self)), self.sa_prune_ratio, self.sa_tome_ver))


def _hook_pyrd(self, layer, hidden_states, position_ids, position_embeddings, start, length, T):
    """Fixed-size pyramid baseline: may fire at several layers, each shrinking the frames further."""
    hidden_states, position_ids, new_len = patch_hooks.pyrd_resize(
        hidden_states, position_ids, start, length, T, self.sa_pyrd_idx2size[layer.self_attn.layer_idx], type(self).sttm_resize_fn)
    self.image_token_length = torch.tensor(new_len)                   # like the reference (:101): persists on the module
    return hidden_states, position_ids, None, _KEEP_IDX


def _hook_quadtree_vl(self, layer, hidden_states, position_ids, position_embeddings, start, length, T):
    hidden_states, position_ids, _cache_pos, idx = patch_hooks.quadtree_merge_qwen2vl(
        hidden_states, position_ids, start, length, T, _item(self.image_H), _item(self.image_W), type(self).sttm_merge_fn,
        *_tree_args(self), slow_ver=self.sttm_slow_ver, merge_into_fn=_fused_merge_fn(type(self)))
    return hidden_states, position_ids, None, idx


def _hook_dycoke_vl(self, layer, hidden_states, position_ids, position_embeddings, start, length, T):
    return _with_new_embeddings(patch_hooks.dycoke_merge(
        hidden_states, position_ids, start, length, T, type(self).sttm_dycoke_fn, self.sa_prune_ratio, gather_positions=True))


def _hook_tome_vl(self, layer, hidden_states, position_ids, position_embeddings, start, length, T):
    return _with_new_embeddings(patch_hooks.tome_merge(
        hidden_states, position_ids, start, length, T, _tome_merge_fn(type(self)), self.sa_prune_ratio, self.sa_tome_ver,
        H=_item(self.image_H), W=_item(self.image_W), gather_positions=True))


def _at_start_layer(self, i, merged):
    return not merged and i == self.sa_start_layer_idx


def _at_pyrd_layers(self, i, merged):
    return i in self.sa_pyrd_llm_idxs


def _batched_hook_qwen2(self, layer, hidden_states, position_ids, pads, attrs):
    starts, lengths, Ts = attrs
    return patch_hooks.quadtree_merge_llava_batched(
        hidden_states, position_ids, pads, starts, lengths, Ts, type(self).sttm_merge_batch_fn, type(self).sttm_pack_fn,
        *_tree_args(self), slow_ver=self.sttm_slow_ver, head_dim=_head_dim(self, layer))


def _batched_hook_qwen2vl(self, layer, hidden_states, position_ids, pads, attrs):
    starts, lengths, Ts, Hs, Ws = attrs
    return patch_hooks.quadtree_merge_qwen2vl_batched(
        hidden_states, position_ids, pads, starts, lengths, Ts, Hs, Ws, type(self).sttm_merge_batch_fn, type(self).sttm_pack_fn,
        *_tree_args(self), slow_ver=self.sttm_slow_ver)


def _positions_qwen2(position_ids, batched, attention_mask, inputs_embeds, past_key_values):
    """(position ids [B or 1, L], no separate text ids)."""
    if position_ids is None and batched:
        position_ids = _positions_from_mask(attention_mask, inputs_embeds)
    if position_ids is None:
        seen = past_key_values.get_seq_length() if past_key_values is not None else 0
        position_ids = (torch.arange(inputs_embeds.shape[1], device=inputs_embeds.device) + seen).unsqueeze(0)
    return position_ids, None


def _positions_qwen2vl(position_ids, batched, attention_mask, inputs_embeds, past_key_values):
    """(3-D mRoPE ids [3, B, L], text ids [B, L] or None): default and 2-D ids are repeated on the three axes, a 4-row tensor is the
    text row followed by the three mRoPE rows."""
    if position_ids is None and batched:
        position_ids = _positions_from_mask(attention_mask, inputs_embeds)[None].expand(3, -1, -1)
    if position_ids is None:
        seen = past_key_values.get_seq_length() if past_key_values is not None else 0
        position_ids = torch.arange(inputs_embeds.shape[1], device=inputs_embeds.device) + seen
        position_ids = position_ids.view(1, 1, -1).expand(3, inputs_embeds.shape[0], -1)
    elif position_ids.ndim == 2:
        position_ids = position_ids[None, ...].expand(3, position_ids.shape[0], -1)
    if position_ids.ndim == 3 and position_ids.shape[0] == 4:
        return position_ids[1:], position_ids[0]
    return position_ids, None


# What differs between the two model families.  `text_ids`: mask creation and the layers receive the text ids (None unless the
# caller passed four rows), not the ids the rotary embedding is computed from.  `hooks`: pattern -> (fires(self, i, merged), hook);
# a pattern that is not in the table takes the "tome" entry, like the reference's else branch.
_Family = namedtuple("_Family", "row_attrs positions text_ids batched_hook hooks layers cache_out dycoke")

_QWEN2 = _Family(
    row_attrs=_QWEN2_ROW_ATTRS, positions=_positions_qwen2, text_ids=False, batched_hook=_batched_hook_qwen2,
    hooks={"quadtree": (_at_start_layer, _hook_quadtree), "quadtree-abl-pos": (_at_start_layer, _hook_quadtree_abl_pos),
           "dycoke-stage1": (_at_start_layer, _hook_dycoke), "dycoke": (_at_start_layer, _hook_dycoke),
           "octree": (_at_start_layer, _hook_octree), "pyrd": (_at_pyrd_layers, _hook_pyrd), "tome": (_at_start_layer, _hook_tome)},
    layers=lambda self: self.layers[: self.config.num_hidden_layers],
    cache_out=lambda past_key_values, use_cache: past_key_values if use_cache else None,
    dycoke=True)

_QWEN2VL = _Family(
    row_attrs=_QWEN2VL_ROW_ATTRS, positions=_positions_qwen2vl, text_ids=True, batched_hook=_batched_hook_qwen2vl,
    hooks={"quadtree": (_at_start_layer, _hook_quadtree_vl), "dycoke-stage1": (_at_start_layer, _hook_dycoke_vl),
           "tome": (_at_start_layer, _hook_tome_vl)},
    layers=lambda self: self.layers,
    cache_out=lambda past_key_values, use_cache: past_key_values,
    dycoke=False)


def _forward(self, fam, input_ids, attention_mask, position_ids, past_key_values, inputs_embeds, use_cache, **kwargs):
    """transformers 5.x decoder forward of either family + the STTM / ToMe hook (prefill).  "quadtree" on B > 1 left-padded prompts
    (or 1-D hook attributes) takes the batched hook; every other case runs the batch-1 hook of the pattern."""
    from transformers.cache_utils import DynamicCache
    from transformers.masking_utils import create_causal_mask, create_sliding_window_causal_mask
    from transformers.modeling_outputs import BaseModelOutputWithPast
    if (input_ids is None) ^ (inputs_embeds is not None):
        raise ValueError("You must specify exactly one of input_ids or inputs_embeds")
    if inputs_embeds is None:
        inputs_embeds = self.embed_tokens(input_ids)
    if use_cache and past_key_values is None:
        past_key_values = DynamicCache(config=self.config)
    prefilling = _is_prefill(past_key_values)
    rows = _batched_rows(self, inputs_embeds, attention_mask, prefilling, fam.row_attrs)
    fires = hook = dycoke_cache = None
    if prefilling:
        _reset_merged_mask(past_key_values)
        if fam.dycoke and past_key_values is not None and getattr(past_key_values, "sttm_dycoke", None) is not None:
            past_key_values.sttm_dycoke = None
        if rows is None and getattr(self, "image_token_length", None) is not None:
            fires, hook = fam.hooks.get(self.sttm_pattern) or fam.hooks["tome"]
            if fam.dycoke and self.sttm_pattern == "dycoke":
                dycoke_cache = past_key_values                        # stage 2 reads what stage 1 leaves there
    elif fam.dycoke and self.sttm_pattern == "dycoke" and (step := _dycoke_step(self, inputs_embeds, past_key_values)) is not None:
        # restored by _qwen2_forward_with_merge
        self.config._sttm_dycoke_step = step
        self.config._attn_implementation = DYCOKE_ATTN
    position_ids, text_position_ids = fam.positions(position_ids, rows is not None, attention_mask, inputs_embeds, past_key_values)
    if not isinstance(mask_map := attention_mask, dict):
        mk = dict(config=self.config, inputs_embeds=inputs_embeds, attention_mask=attention_mask,
                  past_key_values=past_key_values, position_ids=text_position_ids if fam.text_ids else position_ids)
        mask_map = {"full_attention": create_causal_mask(**mk)}
        if getattr(self, "has_sliding_layers", False):
            mask_map["sliding_attention"] = create_sliding_window_causal_mask(**mk)
    # decode after a batched merge: the layers from the merge layer on read the merged layout
    late_masks = None if prefilling else _decode_masks(self, mask_map, inputs_embeds, attention_mask, past_key_values)
    hidden_states = inputs_embeds
    position_embeddings = self.rotary_emb(hidden_states, position_ids)
    merged = False
    for i, layer in enumerate(fam.layers(self)):
        if late_masks is not None and i == self.sa_start_layer_idx:
            mask_map = late_masks
        if rows is not None and not merged and i == self.sa_start_layer_idx:
            L = hidden_states.size(1)
            hidden_states, mask2d, position_ids, idx = fam.batched_hook(self, layer, hidden_states, position_ids, *rows)
            if text_position_ids is not None:
                text_position_ids = _truncate_rows(text_position_ids, rows[0], mask2d, L)
            self.merged_token_1d_idx = idx
            position_embeddings = self.rotary_emb(hidden_states, position_ids)
            mask_map = _merged_layout_masks(self, mask_map, hidden_states, mask2d, None)
            _keep_merged_mask(past_key_values, mask2d, L)
            merged = True
        elif hook is not None and fires(self, i, merged):
            start, length, T = _item(self.image_token_start_index), _item(self.image_token_length), _item(self.num_frame)
            hidden_states, position_ids, position_embeddings, idx = hook(
                self, layer, hidden_states, position_ids, position_embeddings, start, length, T)
            if text_position_ids is not None:
                text_position_ids = text_position_ids[..., :hidden_states.size(1)]
            if idx is not _KEEP_IDX:
                self.merged_token_1d_idx = idx
                merged = True
            if dycoke_cache is not None:
                dycoke_cache.sttm_dycoke = (start, length)            # :370-371: the visual token count BEFORE stage 1
            if position_embeddings is None:
                position_embeddings = self.rotary_emb(hidden_states, position_ids)
            # batch-1 prefill without padding: the shorter sequence is plain causal
            mask_map = _rebuild_masks(self, mask_map, hidden_states)
        hidden_states = layer(hidden_states, attention_mask=mask_map[self.config.layer_types[i]],
                              position_embeddings=position_embeddings,
                              position_ids=text_position_ids if fam.text_ids else position_ids,
                              past_key_values=past_key_values, use_cache=use_cache, **kwargs)
    hidden_states = self.norm(hidden_states)
    return BaseModelOutputWithPast(last_hidden_state=hidden_states, past_key_values=fam.cache_out(past_key_values, use_cache))


def _qwen2_forward_with_merge(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None,
                              inputs_embeds=None, use_cache=None, **kwargs):
    """Qwen2Model.forward + the hook.  A "dycoke" decode step runs with the dispatching attention function and its per-forward
    state on the config; both are put back whatever happens."""
    if self.sttm_pattern != "dycoke":
        return _forward(self, _QWEN2, input_ids, attention_mask, position_ids, past_key_values, inputs_embeds, use_cache, **kwargs)
    x = inputs_embeds if inputs_embeds is not None else input_ids
    if x is not None and x.shape[0] != 1:
        raise NotImplementedError(f"DyCoke reads row 0 of the attention matrix (`[0, -1]`) and prunes one video: batch size 1 only, got {x.shape[0]}")
    cfg = self.config
    saved = cfg._attn_implementation
    try:
        return _forward(self, _QWEN2, input_ids, attention_mask, position_ids, past_key_values, inputs_embeds, use_cache, **kwargs)
    finally:
        if cfg._attn_implementation != saved:
            cfg._attn_implementation = saved
        if getattr(cfg, "_sttm_dycoke_step", None) is not None:
            cfg._sttm_dycoke_step = None


def _qwen2vl_forward_with_merge(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None,
                                inputs_embeds=None, use_cache=None, **kwargs):
    """Qwen2VLTextModel.forward + the hook: 3-D mRoPE position ids are GATHERED by the merged-token index
    (token_merging_qwen2vl_monkey_patch/quadtree_attn_monkey_patch.py:109-113); H and W come from
    `self.image_H / self.image_W` (llava/model/qwen2vl/modeling_qwen2vl.py:1919-1920)."""
    return _forward(self, _QWEN2VL, input_ids, attention_mask, position_ids, past_key_values, inputs_embeds, use_cache, **kwargs)


# ---- installers --------------------------------------------------------------------------------------------------------------
def _qwen2_model_class():
    import transformers.models.qwen2.modeling_qwen2 as m
    return m.Qwen2Model


def _qwen2vl_model_class():
    try:
        import transformers.models.qwen2_vl.modeling_qwen2_vl as m
        return getattr(m, "Qwen2VLTextModel", None) or getattr(m, "Qwen2VLModel", None)
    except Exception:  # noqa: BLE001
        return None


def _install(cls, forward, pattern, attrs, injection_defaults):
    """The class-attribute mechanism of every pattern: configuration as class attributes, injection points (`sttm_*_fn`: tests put
    the CPU oracle there) filled only where absent (`_resolve`), the original forward saved once, `forward` replaced."""
    cls.sttm_pattern = pattern
    for name, value in attrs.items():
        setattr(cls, name, value)
    for name, default in injection_defaults.items():
        if not hasattr(cls, name):
            setattr(cls, name, staticmethod(_resolve(default)))
    if not hasattr(cls, "_sttm_original_forward"):
        cls._sttm_original_forward = cls.forward
    cls.forward = forward


# the batched hook's injection points sit next to `sttm_merge_fn`: the merge of the B videos and the ragged pack
_QUADTREE_FNS = {"sttm_merge_fn": get_quadtree_features, "sttm_merge_batch_fn": get_quadtree_features_batch_reused,
                 "sttm_pack_fn": pack_merged_batch}
_DYCOKE_FNS = {"sttm_dycoke_fn": (".dycoke_merger", "dycoke_ttm")}


def _install_quadtree(cls, forward, pattern, sa_start_layer_idx, sa_tree_thresh, sa_tree_temporal_thresh, sa_tree_root_level,
                      sa_tree_weighted_avg, sttm_slow_ver, **more):
    _install(cls, forward, pattern, dict(
        sa_start_layer_idx=sa_start_layer_idx, sa_tree_thresh=sa_tree_thresh, sa_tree_temporal_thresh=sa_tree_temporal_thresh,
        sa_tree_root_level=sa_tree_root_level, sa_tree_weighted_avg=sa_tree_weighted_avg, sttm_slow_ver=sttm_slow_ver, **more),
        _QUADTREE_FNS)


def replace_qwen2_with_quadtree_attn(sa_start_layer_idx=0, sa_tree_thresh=0.90, sa_tree_temporal_thresh=-1.0,
                                     sa_tree_root_level=0, sa_tree_weighted_avg=False, sttm_slow_ver=False,
                                     sim_per_head=False, **kwargs):
    print("Replace Qwen2 attention path by QuadTree (STTM) token merging [sttm_amd / MI355X]")
    _install_quadtree(_qwen2_model_class(), _qwen2_forward_with_merge, "quadtree", sa_start_layer_idx, sa_tree_thresh,
                      sa_tree_temporal_thresh, sa_tree_root_level, sa_tree_weighted_avg, sttm_slow_ver, sim_per_head=sim_per_head)


def replace_qwen2_with_quadtree_attn_for_abl_pos(sa_start_layer_idx=0, sa_tree_thresh=0.90, sa_tree_temporal_thresh=-1.0,
                                                 sa_tree_root_level=0, sa_tree_weighted_avg=False, sttm_slow_ver=False,
                                                 sim_per_head=False, pos_emb_ver=0, pos_emb_weighted_avg=False, **kwargs):
    """quadtree_attn_monkey_patch_for_abl_pos.py:193-205."""
    print("Replace Qwen2 attention path by QuadTree (STTM) token merging [sttm_amd / MI355X]")
    _install_quadtree(_qwen2_model_class(), _qwen2_forward_with_merge, "quadtree-abl-pos", sa_start_layer_idx, sa_tree_thresh,
                      sa_tree_temporal_thresh, sa_tree_root_level, sa_tree_weighted_avg, sttm_slow_ver, sim_per_head=sim_per_head,
                      pos_emb_ver=pos_emb_ver, pos_emb_weighted_avg=pos_emb_weighted_avg)


def replace_qwen2vl_with_quadtree_attn(sa_start_layer_idx=0, sa_tree_thresh=0.90, sa_tree_temporal_thresh=-1.0,
                                       sa_tree_root_level=0, sa_tree_weighted_avg=False, sttm_slow_ver=False, **kwargs):
    """Qwen2-VL text model (transformers 5.x `Qwen2VLTextModel`): same class-attribute mechanism, forward replaced by
    `_qwen2vl_forward_with_merge` (3-D position-id gather).  No `sim_per_head` here."""
    cls = _qwen2vl_model_class()
    if cls is None:
        return
    print("Replace Qwen2-VL attention path by QuadTree (STTM) token merging [sttm_amd / MI355X]")
    _install_quadtree(cls, _qwen2vl_forward_with_merge, "quadtree", sa_start_layer_idx, sa_tree_thresh, sa_tree_temporal_thresh,
                      sa_tree_root_level, sa_tree_weighted_avg, sttm_slow_ver)


def replace_qwen2_with_octree_attn(sa_start_layer_idx=0, sa_tree_thresh=0.90, sa_tree_root_level=0, **kwargs):
    """octree_attn_monkey_patch.py:163-168."""
    print("Replace Qwen2 attention path by OcTree token merging [sttm_amd / MI355X]")
    _install(_qwen2_model_class(), _qwen2_forward_with_merge, "octree",
             dict(sa_start_layer_idx=sa_start_layer_idx, sa_tree_thresh=sa_tree_thresh, sa_tree_root_level=sa_tree_root_level),
             {"sttm_octree_fn": (".octree_utils", "get_octree_features")})


def replace_qwen2_with_dycoke_stage1_attn(sa_start_layer_idx=0, sa_prune_ratio=0.7, **kwargs):
    """dycoke_stage1_attn_monkey_patch.py:165-169."""
    print("Replace Qwen2 attention path by DyCoke stage-1 pruning [sttm_amd / MI355X]")
    _install(_qwen2_model_class(), _qwen2_forward_with_merge, "dycoke-stage1",
             dict(sa_start_layer_idx=sa_start_layer_idx, sa_prune_ratio=sa_prune_ratio), _DYCOKE_FNS)


def replace_qwen2vl_with_dycoke_stage1_attn(sa_start_layer_idx=0, sa_prune_ratio=0.7, **kwargs):
    """token_merging_qwen2vl_monkey_patch/dycoke_stage1_attn_monkey_patch.py:165-168."""
    cls = _qwen2vl_model_class()
    if cls is None:
        return
    _install(cls, _qwen2vl_forward_with_merge, "dycoke-stage1",
             dict(sa_start_layer_idx=sa_start_layer_idx, sa_prune_ratio=sa_prune_ratio), _DYCOKE_FNS)


def replace_qwen2_with_dycoke_attn(sa_start_layer_idx=0, sa_prune_ratio=0.7, dycoke_l=3, dycoke_p=0.8, **kwargs):
    """dycoke_attn_monkey_patch.py:452-468: stage 1 at prefill, stage 2 (KV selection from layer dycoke_l on) at every decode step."""
    if int(dycoke_l) != dycoke_l or dycoke_l < 1:
        raise ValueError(f"dycoke_l = {dycoke_l} must be an integer >= 1: layer dycoke_l - 1 supplies the attention scores")
    if not 0.0 <= dycoke_p <= 1.0:
        raise ValueError(f"dycoke_p = {dycoke_p} must lie in [0, 1]: int(n0 * (1 - dycoke_p)) visual keys are kept")
    print("Replace Qwen2 attention path by DyCoke (stage 1 + decode-time KV selection) [sttm_amd / MI355X]")
    from transformers.modeling_utils import AttentionInterface
    _install(_qwen2_model_class(), _qwen2_forward_with_merge, "dycoke",
             dict(sa_start_layer_idx=sa_start_layer_idx, sa_prune_ratio=sa_prune_ratio, dycoke_l=int(dycoke_l), dycoke_p=float(dycoke_p)),
             {**_DYCOKE_FNS, **_DECODE_DEFAULTS})
    AttentionInterface.register(DYCOKE_ATTN, _dycoke_attention)


def replace_qwen2_with_pyrd_attn(sa_pyrd_loc_list=[2], sa_pyrd_size_list=[10], **kwargs):
    """pyrd_attn_monkey_patch.py:167-173: resize every frame to size x size (nearest) before the listed decoder layers."""
    print("Replace Qwen2 attention path by Pyramid token merging [sttm_amd / MI355X]")
    assert len(sa_pyrd_loc_list) == len(sa_pyrd_size_list)
    _install(_qwen2_model_class(), _qwen2_forward_with_merge, "pyrd",
             dict(sa_pyrd_llm_idxs=list(sa_pyrd_loc_list), sa_pyrd_idx2size=dict(zip(sa_pyrd_loc_list, sa_pyrd_size_list))),
             {"sttm_resize_fn": (".upstream", "resize_nearest")})


def _install_tome(cls, forward, sa_start_layer_idx, sa_prune_ratio, sa_tome_ver, sa_tome_snippet_size):
    """sa_tome_snippet_size: None = the reference's tome_ver dispatch (where "frame" raises for T > 1); an integer S >= 1 = working
    per-frame (S = 1) / per-snippet ToMe (get_tome_features_snippet)."""
    fns = {"sttm_tome_fn": get_tome_features}
    if sa_tome_snippet_size is not None:
        if isinstance(sa_tome_snippet_size, bool) or int(sa_tome_snippet_size) != sa_tome_snippet_size or sa_tome_snippet_size < 1:
            raise ValueError(f"sa_tome_snippet_size must be an integer >= 1 or None, got {sa_tome_snippet_size!r}")
        sa_tome_snippet_size = int(sa_tome_snippet_size)
        fns["sttm_tome_snippet_fn"] = get_tome_features_snippet
    _install(cls, forward, "tome", dict(sa_start_layer_idx=sa_start_layer_idx, sa_prune_ratio=sa_prune_ratio, sa_tome_ver=sa_tome_ver,
                                        sa_tome_snippet_size=sa_tome_snippet_size), fns)


def replace_qwen2_with_tome_attn(sa_start_layer_idx=0, sa_prune_ratio=0.50, sa_tome_ver="frame", sa_tome_snippet_size=None, **kwargs):
    print("Replace Qwen2 attention path by ToMe token merging [sttm_amd / MI355X]")
    _install_tome(_qwen2_model_class(), _qwen2_forward_with_merge, sa_start_layer_idx, sa_prune_ratio, sa_tome_ver, sa_tome_snippet_size)


def replace_qwen2vl_with_tome_attn(sa_start_layer_idx=0, sa_prune_ratio=0.50, sa_tome_ver="frame", sa_tome_snippet_size=None, **kwargs):
    cls = _qwen2vl_model_class()
    if cls is None:
        return
    print("Replace Qwen2-VL attention path by ToMe token merging [sttm_amd / MI355X]")
    _install_tome(cls, _qwen2vl_forward_with_merge, sa_start_layer_idx, sa_prune_ratio, sa_tome_ver, sa_tome_snippet_size)


def restore_qwen2():
    """Undo replace_qwen2[vl]_with_* (not in the reference; handy for tests)."""
    for cls in (_qwen2_model_class(), _qwen2vl_model_class()):
        if cls is not None and "_sttm_original_forward" in cls.__dict__:
            cls.forward = cls._sttm_original_forward
            del cls._sttm_original_forward
    # "dycoke": the dispatching attention function and the class state of the decode step
    cls = _qwen2_model_class()
    for name in _DECODE_FNS + ("dycoke_l", "dycoke_p"):
        if name in cls.__dict__:
            delattr(cls, name)
    if cls.__dict__.get("sttm_pattern") == "dycoke":
        del cls.sttm_pattern
    from transformers.modeling_utils import AttentionInterface
    AttentionInterface._global_mapping.pop(DYCOKE_ATTN, None)


def replace_qwen2_by_sparse_attn(pattern_name, **kwargs):
    if pattern_name == "quadtree":
        replace_qwen2_with_quadtree_attn(**kwargs)
        replace_qwen2vl_with_quadtree_attn(**kwargs)
    elif pattern_name == "tome":
        replace_qwen2_with_tome_attn(**kwargs)
        replace_qwen2vl_with_tome_attn(**kwargs)
    elif pattern_name == "quadtree-abl-pos":
        replace_qwen2_with_quadtree_attn_for_abl_pos(**kwargs)
    elif pattern_name == "octree":
        replace_qwen2_with_octree_attn(**kwargs)
    elif pattern_name == "pyrd":
        replace_qwen2_with_pyrd_attn(**kwargs)
    elif pattern_name == "dycoke-stage1":
        replace_qwen2_with_dycoke_stage1_attn(**kwargs)
        replace_qwen2vl_with_dycoke_stage1_attn(**kwargs)
    elif pattern_name == "dycoke":
        # the name is routed here together with the test that pins this refusal ("DyCoke stage 2")
        raise NotImplementedError("dycoke is not routed through replace_qwen2_by_sparse_attn yet: install it with "
                                  "replace_qwen2_with_dycoke_attn(sa_start_layer_idx, sa_prune_ratio, dycoke_l, dycoke_p)")
    elif pattern_name in _UNIMPLEMENTED:
        raise NotImplementedError(f"{pattern_name} ({_UNIMPLEMENTED[pattern_name]}) is outside the MI355X hot-path build")
    else:
        raise NotImplementedError(f"{pattern_name} is not yet implemented")
