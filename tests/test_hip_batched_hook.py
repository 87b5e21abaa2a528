"""GPU tests of the batched quadtree hook: the ragged pack kernel (sttm_pack_merged_batch) against its torch restatement, the
batched hook against the per-row batch-1 hook on the device, and greedy `generate` over left-padded batches against every row
run alone."""
import pytest
import torch

from tests._batched_common import installed, left_pad, mrope_batch, prompt_rows, set_one, set_rows
from tests._pack_ref import pack_merged_batch_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _pack_case(B, C, dtype, seed, empty=None):
    """B rows with random geometry (N'_b = 1 on some, empty system or instruction spans on others), random merged rows and tlbr."""
    g = torch.Generator().manual_seed(seed)
    geom, merged = [], []
    for b in range(B):
        T, H, W = [int(v) for v in torch.randint(1, 5, (3,), generator=g)]
        length = T * H * W
        start = 0 if empty == "sys" or b % 3 == 1 else int(torch.randint(0, 6, (1,), generator=g))
        inst = 0 if empty == "inst" or b % 4 == 2 else int(torch.randint(0, 9, (1,), generator=g))
        n = 1 if b % 5 == 0 else int(torch.randint(1, length + 1, (1,), generator=g))
        pad = int(torch.randint(0, 7, (1,), generator=g))
        geom.append([pad, start, length, n, T, H, W, inst])
        rows = n + int(torch.randint(0, 3, (1,), generator=g))                # blocks may hold more rows than N'
        feat = torch.randn(rows, C, generator=g).to(dtype)
        tl = torch.stack([torch.randint(0, T, (rows,), generator=g), torch.randint(0, H, (rows,), generator=g),
                          torch.randint(0, W, (rows,), generator=g)], 1)
        tlbr = torch.cat([tl, tl[:, 1:] + 1], 1).to(torch.int32)
        merged.append((feat.to(DEV), tlbr.to(DEV)))
    L = max(p + s + n_ + i for p, s, n_, _, _, _, _, i in geom) + 2
    for gm in geom:                                        # the instruction span runs to the end of the row: pad absorbs the rest
        gm[0] = L - (gm[1] + gm[2] + gm[7])
    geom = [tuple(gm[:7]) for gm in geom]
    hs = torch.randn(B, L, C, generator=g).to(dtype).to(DEV)
    Lout = max(L - p - n_ + m for p, _, n_, m, _, _, _ in geom) + (seed % 2)
    return hs, merged, geom, Lout


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,C", [(1, 64), (3, 128), (8, 96), (16, 256), (17, 64), (5, 37), (4, 3584)])
@pytest.mark.parametrize("pos_mode", [1, 2])
def test_pack_kernel_is_bit_identical_to_the_restatement(dtype, B, C, pos_mode):
    from sttm_amd.quadtree_interface import pack_merged_batch
    for seed, empty in ((B * 7 + C, None), (B * 7 + C + 1, "sys"), (B * 7 + C + 2, "inst")):
        hs, merged, geom, Lout = _pack_case(B, C, dtype, seed, empty)
        L = hs.shape[1]
        if pos_mode == 1:
            pos = torch.randint(0, 10_000, (B, L), device=DEV)
        else:
            pos = torch.randint(0, 10_000, (3, B, L), device=DEV)
        got = pack_merged_batch(hs, merged, geom, Lout, pos, pos_mode)
        ref = pack_merged_batch_ref(hs, merged, geom, Lout, pos, pos_mode)
        torch.cuda.synchronize()
        assert torch.equal(got[0].view(torch.int8 if dtype == torch.float32 else torch.int16).cpu(),
                           ref[0].view(torch.int8 if dtype == torch.float32 else torch.int16).cpu())
        assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
        assert all(torch.equal(a, b) for a, b in zip(got[3], ref[3]))


def test_pack_takes_broadcast_positions_and_strided_hidden_states():
    from sttm_amd.quadtree_interface import pack_merged_batch
    hs, merged, geom, Lout = _pack_case(6, 64, torch.bfloat16, 3)
    B, L, C = hs.shape
    wide = torch.zeros(B, L, C + 8, dtype=hs.dtype, device=DEV)
    wide[:, :, :C] = hs
    pos = torch.arange(L, device=DEV)[None]
    got = pack_merged_batch(wide[:, :, :C], merged, geom, Lout, pos, 1)
    ref = pack_merged_batch_ref(hs, merged, geom, Lout, pos, 1)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2])
    pos3 = torch.arange(L, device=DEV).view(1, 1, L).expand(3, B, L)
    got = pack_merged_batch(hs, merged, geom, Lout, pos3, 2)
    ref = pack_merged_batch_ref(hs, merged, geom, Lout, pos3, 2)
    assert torch.equal(got[2], ref[2])


LLAVA_ROWS = [(5, 8, 14, 14, 7), (0, 4, 14, 14, 2), (3, 6, 14, 14, 11), (9, 8, 14, 14, 0)]
VL_ROWS = [(5, 3, 10, 18, 7), (0, 4, 14, 14, 2), (3, 2, 18, 10, 11), (1, 3, 10, 18, 4)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("vl", [False, True], ids=["llava", "qwen2vl"])
def test_batched_hook_on_device_is_bit_identical_to_batch1_hooks(dtype, vl):
    from sttm_amd import patch_hooks
    from sttm_amd.quadtree_interface import (get_quadtree_features, get_quadtree_features_batch_reused, get_quadtree_features_into,
                                             pack_merged_batch)
    C = 256
    specs = VL_ROWS if vl else LLAVA_ROWS
    rows = prompt_rows(specs, C, dtype=dtype, device=DEV, seed=4)
    hs, mask = left_pad(rows)
    B, L = mask.shape
    lengths = [r.shape[0] for r in rows]
    pads = [L - n for n in lengths]
    starts, vlen, Ts = [s[0] for s in specs], [s[1] * s[2] * s[3] for s in specs], [s[1] for s in specs]
    for _ in range(2):                                     # the second call reuses the out= blocks of the first
        if vl:
            pos = mrope_batch(lengths, L, DEV)
            out, m2, pos2, idx = patch_hooks.quadtree_merge_qwen2vl_batched(
                hs, pos, pads, starts, vlen, Ts, [s[2] for s in specs], [s[3] for s in specs], get_quadtree_features_batch_reused,
                pack_merged_batch, 0.85, 0.6, 1, False)
        else:
            pos = (mask.cumsum(-1) - 1).masked_fill(mask == 0, 1)
            out, m2, pos2, idx = patch_hooks.quadtree_merge_llava_batched(
                hs, pos, pads, starts, vlen, Ts, get_quadtree_features_batch_reused, pack_merged_batch, 0.85, 0.55, 1, False)
        for b, (spec, r) in enumerate(zip(specs, rows)):
            n_sys, T, H, W, _ = spec
            if vl:
                o1, q1, _, i1 = patch_hooks.quadtree_merge_qwen2vl(r[None], pos[:, b:b + 1, pads[b]:], n_sys, T * H * W, T, H, W,
                                                                   get_quadtree_features, 0.85, 0.6, 1, False,
                                                                   merge_into_fn=get_quadtree_features_into)
                po = out.shape[1] - o1.shape[1]
                assert torch.equal(pos2[:, b, po:], q1[:, 0])
            else:
                o1, q1, i1 = patch_hooks.quadtree_merge_llava(r[None], torch.arange(r.shape[0], device=DEV)[None], n_sys, T * H * W, T,
                                                              get_quadtree_features, 0.85, 0.55, 1, False,
                                                              merge_into_fn=get_quadtree_features_into)
                po = out.shape[1] - o1.shape[1]
                assert torch.equal(pos2[b, po:], q1[0])
            assert torch.equal(out[b, po:], o1[0]) and not out[b, :po].any()
            assert int(m2[b].sum()) == o1.shape[1] and not m2[b, :po].any()
            assert torch.equal(idx[b], i1.to(torch.int32))


def _qwen2_lm(C, dtype, vocab=256):
    from transformers import Qwen2Config, Qwen2ForCausalLM
    torch.manual_seed(0)
    cfg = Qwen2Config(vocab_size=vocab, hidden_size=C, intermediate_size=2 * C, num_hidden_layers=3, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=8192, attn_implementation="sdpa", bos_token_id=1, eos_token_id=2)
    return Qwen2ForCausalLM(cfg).eval().to(DEV, dtype)


def _qwen2vl_lm(C, vocab=256):
    from transformers import Qwen2VLConfig, Qwen2VLForConditionalGeneration
    torch.manual_seed(0)
    cfg = Qwen2VLConfig(text_config=dict(vocab_size=vocab, hidden_size=C, intermediate_size=2 * C, num_hidden_layers=3,
                                         num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=8192,
                                         rope_parameters={"rope_type": "default", "mrope_section": [2, 3, 3], "rope_theta": 10000.0}),
                        vision_config=dict(depth=1, embed_dim=32, hidden_size=C, num_heads=2, in_channels=3, patch_size=2,
                                           spatial_merge_size=1, temporal_patch_size=1))
    cfg._attn_implementation = "sdpa"
    return Qwen2VLForConditionalGeneration(cfg).eval().to(DEV)


@pytest.mark.parametrize("vl", [False, True], ids=["qwen2", "qwen2vl"])
def test_generate_over_a_left_padded_batch_equals_rows_alone(vl):
    pytest.importorskip("transformers")
    from transformers.models.qwen2.modeling_qwen2 import Qwen2Model
    C = 64
    if vl:
        from transformers.models.qwen2_vl.modeling_qwen2_vl import Qwen2VLTextModel
        lm, classes, specs = _qwen2vl_lm(C), [Qwen2VLTextModel, Qwen2Model], [(5, 3, 6, 10, 7), (0, 2, 8, 8, 2), (3, 4, 10, 6, 11),
                                                                             (1, 2, 6, 6, 3)]
        text = lm.model.language_model
    else:
        lm, classes, specs = _qwen2_lm(C, torch.float32), [Qwen2Model], [(5, 4, 8, 8, 7), (0, 3, 8, 8, 2), (3, 2, 8, 8, 11),
                                                                          (2, 4, 8, 8, 1)]
        text = lm.model
    rows = prompt_rows(specs, C, device=DEV)
    hs, mask = left_pad(rows)
    with installed(classes), torch.inference_mode():
        set_rows(text, specs, vl)
        out = lm.generate(inputs_embeds=hs, attention_mask=mask, max_new_tokens=8, do_sample=False, pad_token_id=0)
        assert isinstance(text.merged_token_1d_idx, list) and len(text.merged_token_1d_idx) == len(specs)
        for b, (spec, r) in enumerate(zip(specs, rows)):
            set_one(text, spec, vl)
            one = lm.generate(inputs_embeds=r[None], attention_mask=torch.ones(1, r.shape[0], dtype=torch.long, device=DEV),
                              max_new_tokens=8, do_sample=False, pad_token_id=0)
            assert torch.equal(one[0], out[b]), (b, one, out[b])


def test_bf16_teacher_forced_logits_match_rows_alone():
    """bf16: per-row logits of a padded batch (prefill + 3 teacher-forced steps) within 0.05 of each row alone (bf16 GEMMs over a
    different key count round differently; the merged rows themselves are bit-identical, see above)."""
    pytest.importorskip("transformers")
    from transformers.models.qwen2.modeling_qwen2 import Qwen2Model
    C = 128
    lm = _qwen2_lm(C, torch.bfloat16)
    specs = [(5, 4, 8, 8, 7), (0, 3, 8, 8, 2), (3, 2, 8, 8, 11), (2, 4, 8, 8, 1)]
    rows = prompt_rows(specs, C, dtype=torch.bfloat16, device=DEV)
    hs, mask = left_pad(rows)
    B = len(rows)
    lengths = [r.shape[0] for r in rows]
    toks = torch.randint(3, 256, (3, B), generator=torch.Generator().manual_seed(1)).to(DEV)
    with installed([Qwen2Model]), torch.inference_mode():
        set_rows(lm.model, specs)
        res = lm(inputs_embeds=hs, attention_mask=mask, position_ids=(mask.cumsum(-1) - 1).masked_fill(mask == 0, 1), use_cache=True)
        logits = [res.logits[:, -1].float()]
        cache, m = res.past_key_values, mask
        for t in range(3):
            m = torch.cat([m, torch.ones(B, 1, dtype=m.dtype, device=DEV)], 1)
            p = torch.tensor([[n + t] for n in lengths], device=DEV)
            res = lm(input_ids=toks[t][:, None], attention_mask=m, position_ids=p, past_key_values=cache, use_cache=True)
            logits.append(res.logits[:, -1].float())
        for b, (spec, r) in enumerate(zip(specs, rows)):
            set_one(lm.model, spec)
            res = lm(inputs_embeds=r[None], use_cache=True)
            one = [res.logits[0, -1].float()]
            cache1 = res.past_key_values
            for t in range(3):
                res = lm(input_ids=toks[t][b].view(1, 1), position_ids=torch.tensor([[lengths[b] + t]], device=DEV),
                         past_key_values=cache1, use_cache=True)
                one.append(res.logits[0, -1].float())
            for t in range(4):
                err = float((logits[t][b] - one[t]).abs().max())
                assert err <= 0.05, (b, t, err)
