"""Shared pieces of the batched-hook tests: tiny Qwen2 / Qwen2-VL text models, left-padded batches of video prompts, and the
batch-1 forward of one row with the hook installed."""
import contextlib

import torch

from sttm_amd import monkey_patch_interface as MPI
from sttm_amd.synth import synth_video

THRESH = dict(sa_tree_thresh=0.85, sa_tree_temporal_thresh=0.55, sa_tree_root_level=1)


def qwen2_model(C=32, layers=3, attn="sdpa", seed=0, vocab=64):
    from transformers import Qwen2Config
    from transformers.models.qwen2.modeling_qwen2 import Qwen2Model
    torch.manual_seed(seed)
    cfg = Qwen2Config(vocab_size=vocab, hidden_size=C, intermediate_size=2 * C, num_hidden_layers=layers, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=8192, attn_implementation=attn)
    return Qwen2Model(cfg).eval()


def qwen2vl_text_config(C=32, layers=3, attn="sdpa", vocab=64):
    from transformers.models.qwen2_vl.configuration_qwen2_vl import Qwen2VLTextConfig
    cfg = Qwen2VLTextConfig(vocab_size=vocab, hidden_size=C, intermediate_size=2 * C, num_hidden_layers=layers, num_attention_heads=4,
                            num_key_value_heads=2, max_position_embeddings=8192,
                            rope_parameters={"rope_type": "default", "mrope_section": [1, 1, 2], "rope_theta": 10000.0})
    cfg._attn_implementation = attn
    return cfg


def qwen2vl_model(C=32, layers=3, attn="sdpa", seed=0):
    from transformers.models.qwen2_vl.modeling_qwen2_vl import Qwen2VLTextModel
    torch.manual_seed(seed)
    return Qwen2VLTextModel(qwen2vl_text_config(C, layers, attn)).eval()


def prompt_rows(specs, C, dtype=torch.float32, device="cpu", seed=0):
    """specs: (n_sys, T, H, W, n_inst) per row -> list of [L_b, C] unpadded prompts (video tokens channels-last in the middle)."""
    rows = []
    g = torch.Generator().manual_seed(seed + 100)
    for k, (n_sys, T, H, W, n_inst) in enumerate(specs):
        vis = synth_video(T, C, H, W, seed=seed + k).permute(0, 2, 3, 1).reshape(T * H * W, C)
        rows.append(torch.cat([torch.randn(n_sys, C, generator=g), vis, torch.randn(n_inst, C, generator=g)]).to(device, dtype))
    return rows


def left_pad(rows, extra_pad=(), seed=7):
    """Stack [L_b, C] rows into [B, L, C] with random pad embeddings in front (pads must not leak) and the 2-D mask."""
    B = len(rows)
    L = max(r.shape[0] + (extra_pad[b] if b < len(extra_pad) else 0) for b, r in enumerate(rows))
    C = rows[0].shape[1]
    g = torch.Generator().manual_seed(seed)
    hs = torch.randn(B, L, C, generator=g).to(rows[0].device, rows[0].dtype)
    mask = torch.zeros(B, L, dtype=torch.long, device=rows[0].device)
    for b, r in enumerate(rows):
        hs[b, L - r.shape[0]:] = r
        mask[b, L - r.shape[0]:] = 1
    return hs, mask


def positions_1d(mask):
    return (mask.cumsum(-1) - 1).masked_fill(mask == 0, 1)


def mrope_ids(n, device="cpu"):
    """A 3-D id pattern of an n-token prompt whose three axes differ (so that a truncation would show)."""
    a = torch.arange(n, device=device)
    return torch.stack([a, 1000 + a // 2, 5000 + a // 3])                                         # [3, n]


def mrope_batch(lengths, L, device="cpu"):
    pos = torch.ones(3, len(lengths), L, dtype=torch.long, device=device)
    for b, n in enumerate(lengths):
        pos[:, b, L - n:] = mrope_ids(n, device)
    return pos


def set_rows(model, specs, vl=False, as_tensor_rows=True):
    starts = [s[0] for s in specs]
    lengths = [s[1] * s[2] * s[3] for s in specs]
    Ts = [s[1] for s in specs]
    model.image_token_start_index = torch.tensor(starts)
    model.image_token_length = torch.tensor(lengths)
    model.num_frame = torch.tensor(Ts)
    if vl:
        model.image_H = torch.tensor([s[2] for s in specs])
        model.image_W = torch.tensor([s[3] for s in specs])


def set_one(model, spec, vl=False):
    n_sys, T, H, W, _ = spec
    model.image_token_start_index = torch.tensor(n_sys)
    model.image_token_length = torch.tensor(T * H * W)
    model.num_frame = torch.tensor(T)
    if vl:
        model.image_H = torch.tensor(H)
        model.image_W = torch.tensor(W)


@contextlib.contextmanager
def installed(classes, merge_fn=None, merge_batch_fn=None, pack_fn=None, sa_start_layer_idx=1, **kw):
    """replace_qwen2_by_sparse_attn("quadtree") with optional injected functions; everything undone on exit."""
    injected = []
    try:
        MPI.replace_qwen2_by_sparse_attn("quadtree", sa_start_layer_idx=sa_start_layer_idx, **{**THRESH, **kw})
        for cls in classes:
            for name, fn in (("sttm_merge_fn", merge_fn), ("sttm_merge_batch_fn", merge_batch_fn), ("sttm_pack_fn", pack_fn)):
                if fn is not None:
                    setattr(cls, name, staticmethod(fn))
                    injected.append((cls, name))
        yield
    finally:
        MPI.restore_qwen2()
        for cls in classes:
            for name in ("sttm_merge_fn", "sttm_merge_batch_fn", "sttm_pack_fn"):
                if name in cls.__dict__:
                    delattr(cls, name)
