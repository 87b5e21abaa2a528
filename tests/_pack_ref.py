"""Torch restatement of the ragged pack of the batched quadtree hook (sttm_pack_merged_batch, include/sttm_hip.h), written from the
batch-1 hook it must agree with (patch_hooks.quadtree_merge_llava / _qwen2vl): per row, system ++ merged rows ++ instruction,
left-padded to Lout with zero rows; positions truncated (mode 1) or 3-D ids gathered by the merged index (mode 2); pads get 1."""
import torch


def pack_merged_batch_ref(hidden_states, merged, geom, Lout, position_ids=None, pos_mode=0):
    B, L, C = hidden_states.shape
    dev = hidden_states.device
    out = torch.zeros((B, Lout, C), dtype=hidden_states.dtype, device=dev)
    mask = torch.zeros((B, Lout), dtype=torch.int64, device=dev)
    pos = None
    if pos_mode == 1:
        pin = position_ids.to(torch.int64).expand(B, L)
        pos = torch.ones((B, Lout), dtype=torch.int64, device=dev)
    elif pos_mode == 2:
        pin = position_ids.to(torch.int64).expand(3, B, L)
        pos = torch.ones((3, B, Lout), dtype=torch.int64, device=dev)
    idxs = []
    for b, ((feat, tlbr), (pad, start, length, n, T, H, W)) in enumerate(zip(merged, geom)):
        end = pad + start + length
        lb = L - pad - length + n
        po = Lout - lb
        out[b, po:] = torch.cat([hidden_states[b, pad:pad + start], feat[:n], hidden_states[b, end:]])
        mask[b, po:] = 1
        t = tlbr[:n].to(torch.int64)
        idx = t[:, 0] * (H * W) + t[:, 1] * W + t[:, 2]
        if pos_mode == 1:
            pos[b, po:] = pin[b, pad:pad + lb]
        elif pos_mode == 2:
            seg = pin[:, b, pad:]
            pos[:, b, po:] = torch.cat([seg[:, :start], seg[:, start:start + length][:, idx], seg[:, start + length:]], dim=-1)
        idxs.append(idx.to(torch.int32))
    return out, mask, pos, idxs
