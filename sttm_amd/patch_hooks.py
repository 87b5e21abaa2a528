"""Tensor glue of the reference's patched decoder forward, as plain functions.

These restate the ~25 lines the reference inserts before decoder layer `sa_start_layer_idx` during prefill:
    LLaVA-Video / OneVision  token_merging_monkey_patch/quadtree_attn_monkey_patch.py:88-117
    Qwen2-VL                 token_merging_qwen2vl_monkey_patch/quadtree_attn_monkey_patch.py:88-115
    ToMe                     token_merging_monkey_patch/tome_attn_monkey_patch.py:88-107
The visual slice is handed to the merge function as a [T, C, H, W] *view* of [T, H, W, C] memory (no copy),
exactly like einops.rearrange(visual[0], "(T H W) C -> T C H W") in the reference.
"""
import math

import torch


def _video_view(visual, T, H, W):
    C = visual.shape[-1]
    return visual.reshape(T, H, W, C).permute(0, 3, 1, 2)


def split_prompt(hidden_states, start, length):
    end = start + length
    return hidden_states[:, :start], hidden_states[:, start:end], hidden_states[:, end:]


def _splice(hidden_states, start, length, feat):
    """system ++ feat ++ instruction: the rows feat [N', C] in place of the visual slice."""
    sys_f, _, inst_f = split_prompt(hidden_states, start, length)
    return torch.cat([sys_f, feat.unsqueeze(0), inst_f], dim=1)


def _positions_after(position_ids, start, length, n, idx=None):
    """Position ids of the spliced sequence of n tokens.  idx None: [B, S] ids TRUNCATED to n.  Otherwise the visual columns are
    GATHERED by idx along the last axis ([B, S] or 3-D mRoPE [3, B, S] ids), system / instruction ids kept."""
    if idx is None:
        return position_ids[:, :n]
    end = start + length
    return torch.cat([position_ids[..., :start], position_ids[..., start:end][..., idx.long()], position_ids[..., end:]], dim=-1)


def _merge_concat(hidden_states, start, length, video, merge_fn, merge_into_fn, args, kwargs):
    """system ++ merge(video) ++ instruction  (quadtree_attn_monkey_patch.py:101-105).

    With `merge_into_fn` (sttm_amd.get_quadtree_features_into) the merged rows are written by the kernels straight into
    the new hidden-state buffer: no intermediate [N', C] tensor and no copy of it by torch.cat.
    The new buffer has the OLD sequence length (N' <= length), the result is its leading [:, :S'] view."""
    sys_f, _, inst_f = split_prompt(hidden_states, start, length)
    if merge_into_fn is None or hidden_states.size(0) != 1:
        feat, npatch, tlbr = merge_fn(video, *args, **kwargs)
        return torch.cat([sys_f, feat.unsqueeze(0), inst_f], dim=1), tlbr, None
    new = torch.empty_like(hidden_states, memory_format=torch.contiguous_format)
    new[:, :start].copy_(sys_f)
    # the kernels also write merged_token_1d_idx (t*H*W + y1*W + x1, :103-104) when the merge function offers it: three
    # elementwise launches of the caller less
    idx = None
    if getattr(merge_into_fn, "returns_idx", False):
        feat, npatch, tlbr, idx = merge_into_fn(new[0, start:], video, *args, return_idx=True, **kwargs)
    else:
        feat, npatch, tlbr = merge_into_fn(new[0, start:], video, *args, **kwargs)
    n = feat.size(0)
    new[:, start + n:start + n + inst_f.size(1)].copy_(inst_f)
    return new[:, :start + n + inst_f.size(1)], tlbr, idx


def quadtree_merge_llava(hidden_states, position_ids, start, length, T, merge_fn, threshold, temporal_thresh,
                         root_level, weighted_avg, slow_ver=False, head_dim=None, merge_into_fn=None):
    """Returns (merged hidden_states [1, S', C], position_ids[:, :S'], merged_token_1d_idx)."""
    H = W = int(math.sqrt(length // T))                                   # :97 (needs mm_newline_position=no_token)
    video = _video_view(hidden_states[0, start:start + length], T, H, W)
    merged, tlbr, idx = _merge_concat(hidden_states, start, length, video, merge_fn, merge_into_fn,
                                      (threshold, temporal_thresh, root_level, weighted_avg),
                                      dict(slow_ver=slow_ver, head_dim=head_dim))
    if idx is None:
        idx = tlbr[:, 0] * (H * W) + tlbr[:, 1] * W + tlbr[:, 2]          # :103-104
    return merged, position_ids[:, :merged.size(1)], idx                   # :114 (truncate, not gather)


def quadtree_merge_qwen2vl(hidden_states, position_ids, start, length, T, H, W, merge_fn, threshold, temporal_thresh,
                           root_level, weighted_avg, slow_ver=False, merge_into_fn=None):
    """position_ids is the 3-D mRoPE tensor [3, B, S]; the visual part is GATHERED by the merged index (:109-113).
    Returns (merged hidden_states, position_ids, cache_position, merged_token_1d_idx)."""
    end = start + length
    video = _video_view(hidden_states[0, start:end], T, H, W)
    merged, tlbr, idx = _merge_concat(hidden_states, start, length, video, merge_fn, merge_into_fn,
                                      (threshold, temporal_thresh, root_level, weighted_avg), dict(slow_ver=slow_ver))
    if idx is None:
        idx = tlbr[:, 0] * (H * W) + tlbr[:, 1] * W + tlbr[:, 2]
    pos = _positions_after(position_ids, start, length, merged.size(1), idx)
    cache_position = torch.arange(merged.size(1), device=merged.device, dtype=torch.int)      # :114
    return merged, pos, cache_position, idx


# ---- batched prompts (B >= 1 left-padded rows, one video per row) ------------------------------------------------------------
# Row b's indices count from its first valid token, pads[b] columns in: the same numbers a batch-1 call of that row would use.
# merge_batch_fn(videos, threshold, temporal_thresh, root_level, weighted_avg, slow_ver=, head_dim=) -> B (features, num_patches, tlbr)
# (sttm_amd.quadtree_interface.get_quadtree_features_batch_reused on the device); pack_fn(hidden_states, merged, geom, Lout, position_ids,
# pos_mode) -> (hidden [B, Lout, C], key mask [B, Lout], position ids, B merged_token_1d_idx) (quadtree_interface.pack_merged_batch).
POS_TRUNCATE, POS_GATHER3 = 1, 2         # STTM_PACK_POS_* of include/sttm_hip.h


def _merge_and_pack(hidden_states, position_ids, rows, merge_batch_fn, pack_fn, merge_args, merge_kwargs, pos_mode):
    """rows: B tuples (pad, start, length, T, H, W).  One batched merge of the B videos, then one pack into the compact block
    [B, L'max, C] with L'_b = L - pad_b - length_b + N'_b (N'_b is known on the host once the merge returns)."""
    L = hidden_states.size(1)
    videos = [_video_view(hidden_states[b, p + s:p + s + n], T, H, W) for b, (p, s, n, T, H, W) in enumerate(rows)]
    res = merge_batch_fn(videos, *merge_args, **merge_kwargs)
    geom = [(p, s, n, int(feat.size(0)), T, H, W) for (p, s, n, T, H, W), (feat, _, _) in zip(rows, res)]
    Lout = max(L - p - n + m for p, _, n, m, _, _, _ in geom)
    return pack_fn(hidden_states, [(feat, tlbr) for feat, _, tlbr in res], geom, Lout, position_ids, pos_mode)


def quadtree_merge_llava_batched(hidden_states, position_ids, pads, starts, lengths, Ts, merge_batch_fn, pack_fn, threshold,
                                 temporal_thresh, root_level, weighted_avg, slow_ver=False, head_dim=None):
    """quadtree_merge_llava on every row of a left-padded batch [B, L, C]; position_ids [B or 1, L] are TRUNCATED per row (:114).
    Returns (hidden_states [B, L'max, C], key mask [B, L'max] int64, position_ids [B, L'max], list of B merged_token_1d_idx)."""
    rows = []
    for p, s, n, T in zip(pads, starts, lengths, Ts):
        H = int(math.sqrt(n // T))                                        # :97
        rows.append((p, s, n, T, H, H))
    return _merge_and_pack(hidden_states, position_ids, rows, merge_batch_fn, pack_fn,
                           (threshold, temporal_thresh, root_level, weighted_avg), dict(slow_ver=slow_ver, head_dim=head_dim),
                           POS_TRUNCATE)


def quadtree_merge_qwen2vl_batched(hidden_states, position_ids, pads, starts, lengths, Ts, Hs, Ws, merge_batch_fn, pack_fn, threshold,
                                   temporal_thresh, root_level, weighted_avg, slow_ver=False):
    """quadtree_merge_qwen2vl on every row of a left-padded batch: the 3-D mRoPE ids [3, B or 1, L] of every row are GATHERED by its
    merged index, system / instruction ids kept (:109-113).  Returns (hidden_states [B, L'max, C], key mask [B, L'max] int64,
    position_ids [3, B, L'max], list of B merged_token_1d_idx)."""
    rows = list(zip(pads, starts, lengths, Ts, Hs, Ws))
    return _merge_and_pack(hidden_states, position_ids, rows, merge_batch_fn, pack_fn,
                           (threshold, temporal_thresh, root_level, weighted_avg), dict(slow_ver=slow_ver), POS_GATHER3)


def tome_merge(hidden_states, position_ids, start, length, T, merge_fn, prune_ratio, tome_ver, H=None, W=None,
               gather_positions=False):
    """ToMe hook.  LLaVA (token_merging_monkey_patch/tome_attn_monkey_patch.py:88-107): H = W = sqrt(len / T), position_ids
    [B, S] are TRUNCATED to the new length (:105).  Qwen2-VL (token_merging_qwen2vl_monkey_patch/tome_attn_monkey_patch.py:
    88-111, gather_positions=True): H, W come from the module, and the 3-D mRoPE ids [3, B, S] of the visual part are
    GATHERED by the ToMe token index, system / instruction ids kept (:105-108)."""
    if H is None:
        H = int(math.sqrt(length // T))
        W = (length // T) // H
    video = _video_view(hidden_states[0, start:start + length], T, H, W)
    feat, token_idx = merge_fn(video, prune_ratio, tome_ver)
    merged = _splice(hidden_states, start, length, feat)
    return merged, _positions_after(position_ids, start, length, merged.size(1), token_idx if gather_positions else None), token_idx


def pyrd_resize(hidden_states, position_ids, start, length, T, tgt_size, resize_fn):
    """The "pyrd" baseline (pyrd_attn_monkey_patch.py:88-112): every frame of the visual slice is resized to
    tgt_size x tgt_size with F.interpolate's default (nearest) mode.  resize_fn(tokens [T, H*W, C], H, W, (s, s)).
    Returns (hidden_states, position_ids[:, :S'], new visual length)."""
    H = int(math.sqrt(length // T))                                       # :97
    C = hidden_states.shape[-1]
    resized = resize_fn(hidden_states[0, start:start + length].reshape(T, H * H, C), H, H, (tgt_size, tgt_size))
    resized = resized.reshape(T * tgt_size * tgt_size, C)
    merged = _splice(hidden_states, start, length, resized)               # :103
    return merged, _positions_after(position_ids, start, length, merged.size(1)), resized.size(0)       # :101, :108


def dycoke_merge(hidden_states, position_ids, start, length, T, ttm_fn, prune_ratio, gather_positions=False):
    """DyCoke stage-1 hook: LLaVA (dycoke_stage1_attn_monkey_patch.py:88-107) truncates position_ids; Qwen2-VL
    (token_merging_qwen2vl_monkey_patch/dycoke_stage1_attn_monkey_patch.py:88-108, gather_positions=True) gathers the 3-D
    mRoPE ids of the kept tokens.  ttm_fn(tokens [T*P, C], T, prune_ratio) -> (tokens, flat ids)."""
    feat, idx = ttm_fn(hidden_states[0, start:start + length], T, prune_ratio)
    merged = _splice(hidden_states, start, length, feat)
    return merged, _positions_after(position_ids, start, length, merged.size(1), idx if gather_positions else None), idx


def octree_merge(hidden_states, position_ids, start, length, T, octree_fn, threshold, root_level):
    """Octree hook (octree_attn_monkey_patch.py:87-106): features only, position_ids truncated."""
    H = int(math.sqrt(length // T))                                       # :96
    video = _video_view(hidden_states[0, start:start + length], T, H, H)
    merged = _splice(hidden_states, start, length, octree_fn(video, threshold, root_level))
    return merged, _positions_after(position_ids, start, length, merged.size(1))


def quadtree_merge_abl_pos(hidden_states, position_ids, position_embeddings, start, length, T, merge_fn, threshold,
                           temporal_thresh, root_level, weighted_avg, pos_emb_ver, pos_emb_weighted_avg, rotary_fn,
                           slow_ver=False, head_dim=None):
    """Position-embedding ablation hook (quadtree_attn_monkey_patch_for_abl_pos.py:88-136).
    pos_emb_ver 0: re-number the shorter sequence (the standard hook); 1: merge the RoPE (cos, sin) rows alongside the features
    (`pos_embs=`); 2: keep every merged token's ORIGINAL position id (gather by the merged index).
    rotary_fn(hidden_states, position_ids) -> (cos, sin).  Returns (hidden_states, position_ids, position_embeddings, idx)."""
    end = start + length
    H = W = int(math.sqrt(length // T))                                   # :97
    video = _video_view(hidden_states[0, start:end], T, H, W)
    pos_video = None
    if pos_emb_ver > 0:                                                   # :100-104
        pos_video = tuple(_video_view(p[0, start:end], T, H, W) for p in position_embeddings)
    res = merge_fn(video, threshold, temporal_thresh, root_level, weighted_avg, slow_ver=slow_ver, head_dim=head_dim,
                   pos_embs=pos_video, pos_emb_weighted_avg=pos_emb_weighted_avg)
    if pos_emb_ver > 0:
        feat, _, tlbr, merged_pos = res
    else:
        feat, _, tlbr = res
    idx = tlbr[:, 0] * (H * W) + tlbr[:, 1] * W + tlbr[:, 2]              # :113-114
    merged = _splice(hidden_states, start, length, feat)
    n = merged.size(1)
    if pos_emb_ver == 0:                                                  # :120-123
        position_ids = _positions_after(position_ids, start, length, n)
        position_embeddings = rotary_fn(merged, position_ids)
    elif pos_emb_ver == 1:                                                # :124-128
        position_embeddings = tuple(_splice(p, start, length, mp) for p, mp in zip(position_embeddings, merged_pos))
        position_ids = _positions_after(position_ids, start, length, n)
    elif pos_emb_ver == 2:                                                # :129-135
        position_ids = _positions_after(position_ids, start, length, n, idx)
        position_embeddings = rotary_fn(merged, position_ids)
    return merged, position_ids, position_embeddings, idx
