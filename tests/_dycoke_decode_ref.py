"""Torch restatement of DyCoke stage 2 as the reference writes it (token_merging_monkey_patch/dycoke_attn_monkey_patch.py; the line
numbers below are that file's).  The file itself cannot be imported under transformers 5.x, so the cited lines are restated here with
the same operations in the same order.  Everything computes in the dtype it is given; run on float64 inputs it is the yardstick.

Shapes are those an attention function of transformers 5.x sees at a decode step: query [1, Hq, 1, D] (post-RoPE), key / value
[1, Hkv, Lk, D] (what `cache.update` returned, the new token included).

Two things are pinned down where the reference leaves them open or overruns:
  * `torch.topk` (:69) does not specify which of several equal scores it takes; here ties go to the smaller index (stable sort).
  * the tail `full_range[start + n0:]` (:72-74) runs to `seq_length_with_past`, one past the end of the cache for dycoke_l >= 1
    (:402-404 add the query length to a cache that already holds it); here it is clipped to Lk.
The kept window indices are returned in ascending order (the reference keeps topk's order, `sorted=False`: any order; attention over
a set of keys does not depend on it).
"""
import torch


def repeat_kv(x, n_rep):
    """transformers' repeat_kv: [1, Hkv, L, D] -> [1, Hkv * n_rep, L, D], query head h reads KV head h // n_rep."""
    return x if n_rep == 1 else x.repeat_interleave(n_rep, dim=1)


def decode_attn_scores_ref(query, key, scaling):
    """:410-411 (eager layer dycoke_l - 1 with output_attentions) and :80 `attn[1].mean(1)[0, -1]` -> score [Lk]."""
    G = query.shape[1] // key.shape[1]
    attn = torch.matmul(query, repeat_kv(key, G).transpose(2, 3)) * scaling          # eager attention, no mask at batch 1 / query 1
    attn = torch.softmax(attn, dim=-1)                                                # [1, Hq, 1, Lk]
    return attn.mean(1)[0, -1]                                                        # :80


def num_keep_of(n0, dycoke_p):
    return int(n0 * (1 - dycoke_p))                                                   # :66


def select_keep_ref(score, start, n0, num_keep):
    """:81-83 (the window) and update_cache :62-77 -> keep [start + num_keep + tail] int64."""
    Lk = score.shape[0]
    image_attention = score[start:start + n0]                                         # :83 (slicing clips at Lk)
    if num_keep > image_attention.shape[0]:
        raise RuntimeError("selected index k out of range")                           # what topk raises (:69)
    order = torch.sort(image_attention, descending=True, stable=True)[1][:num_keep]   # :69, ties to the smaller index
    top_indices = torch.sort(order)[0] + start
    full_range = torch.arange(Lk, device=score.device)                                # :73, clipped to Lk
    return torch.cat([full_range[:start], top_indices, full_range[start + n0:]])      # :74


def gathered_decode_attention_ref(query, key, value, keep, scaling):
    """PrunableDynamicCache.update :54-60 (gather K and V by the keep list) and the attention over them -> [1, 1, Hq, D]."""
    idx = keep.to(torch.int64)
    k = key.index_select(2, idx)                                                      # :58 (torch.gather over expanded indices)
    v = value.index_select(2, idx)                                                    # :59
    G = query.shape[1] // k.shape[1]
    attn = torch.softmax(torch.matmul(query, repeat_kv(k, G).transpose(2, 3)) * scaling, dim=-1)
    return torch.matmul(attn, repeat_kv(v, G)).transpose(1, 2).contiguous()


def as_decode_fns(record=None):
    """The three injection points of the patched forward bound to the restatement (`sttm_decode_*_fn`); `record`, a list, receives
    every keep list."""
    def select(score, start, n0, num_keep):
        keep = select_keep_ref(score, start, n0, num_keep)
        if record is not None:
            record.append(keep.clone())
        return keep
    return decode_attn_scores_ref, select, gathered_decode_attention_ref
