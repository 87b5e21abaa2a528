"""The batched quadtree hook on the CPU: the CPU oracle merges the videos and tests/_pack_ref.py restates the pack, both injected
through the class attributes next to `sttm_merge_fn`.  Every row of a left-padded batch must give what the batch-1 hook gives on
that row's unpadded prompt: merged rows, merged_token_1d_idx, masks and position ids exactly, last hidden states within fp32
noise, at prefill and on teacher-forced decode steps.  Also: argument checks of sttm_pack_merged_batch and the resources of its
kernels in the built library."""
import ctypes
import os

import pytest
import torch

from oracle import sttm_oracle as O
from sttm_amd import patch_hooks
from tests._batched_common import (installed, left_pad, mrope_batch, mrope_ids, positions_1d, prompt_rows, qwen2_model,
                                   qwen2vl_model, set_one, set_rows)
from tests._pack_ref import pack_merged_batch_ref

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sttm_amd", "lib", "libsttm_hip.so")

# (n_sys, T, H, W, n_inst): different pads, instruction lengths, T; an empty system span
LLAVA_ROWS = [(5, 4, 8, 8, 7), (0, 3, 8, 8, 2), (3, 2, 8, 8, 11)]
VL_ROWS = [(5, 3, 6, 10, 7), (0, 2, 8, 8, 2), (3, 4, 10, 6, 11)]


def oracle_batch(videos, *args, **kw):
    return [O.get_quadtree_features(v, *args, **kw) for v in videos]


def test_llava_glue_matches_batch1_rows():
    rows = prompt_rows(LLAVA_ROWS, 16)
    hs, mask = left_pad(rows, extra_pad=(0, 5))
    pos = positions_1d(mask)
    B, L = mask.shape
    pads = (L - mask.sum(-1)).tolist()
    out, m2, pos2, idx = patch_hooks.quadtree_merge_llava_batched(
        hs, pos, pads, [r[0] for r in LLAVA_ROWS], [r[1] * r[2] * r[3] for r in LLAVA_ROWS], [r[1] for r in LLAVA_ROWS],
        oracle_batch, pack_merged_batch_ref, 0.85, 0.55, 1, False)
    assert len(idx) == B and out.shape[:2] == m2.shape == pos2.shape
    for b, (spec, r) in enumerate(zip(LLAVA_ROWS, rows)):
        n_sys, T = spec[0], spec[1]
        p1 = torch.arange(r.shape[0]).unsqueeze(0)
        o1, q1, i1 = patch_hooks.quadtree_merge_llava(r[None], p1, n_sys, T * 64, T, O.get_quadtree_features, 0.85, 0.55, 1, False)
        n = o1.shape[1]
        po = out.shape[1] - n
        assert torch.equal(out[b, po:], o1[0]) and torch.equal(out[b, :po], torch.zeros_like(out[b, :po]))
        assert torch.equal(m2[b], (torch.arange(out.shape[1]) >= po).long())
        assert torch.equal(pos2[b, po:], q1[0])
        assert torch.equal(idx[b].long(), i1.long()) and idx[b].dtype == torch.int32
    assert out.shape[1] == max(int(m2[b].sum()) for b in range(B))                # L'max: the longest row has no pad


def test_qwen2vl_glue_gathers_3d_ids_per_row():
    rows = prompt_rows(VL_ROWS, 16, seed=3)
    hs, mask = left_pad(rows)
    B, L = mask.shape
    lengths = [r.shape[0] for r in rows]
    pos = mrope_batch(lengths, L)
    pads = [L - n for n in lengths]
    out, m2, pos2, idx = patch_hooks.quadtree_merge_qwen2vl_batched(
        hs, pos, pads, [r[0] for r in VL_ROWS], [r[1] * r[2] * r[3] for r in VL_ROWS], [r[1] for r in VL_ROWS],
        [r[2] for r in VL_ROWS], [r[3] for r in VL_ROWS], oracle_batch, pack_merged_batch_ref, 0.85, 0.6, 1, False)
    assert pos2.shape == (3, B, out.shape[1])
    for b, (spec, r) in enumerate(zip(VL_ROWS, rows)):
        n_sys, T, H, W, _ = spec
        o1, q1, _, i1 = patch_hooks.quadtree_merge_qwen2vl(r[None], mrope_ids(r.shape[0])[:, None], n_sys, T * H * W, T, H, W,
                                                           O.get_quadtree_features, 0.85, 0.6, 1, False)
        po = out.shape[1] - o1.shape[1]
        assert torch.equal(out[b, po:], o1[0])
        assert torch.equal(pos2[:, b, po:], q1[:, 0]) and torch.equal(pos2[:, b, :po], torch.ones_like(pos2[:, b, :po]))
        assert torch.equal(idx[b].long(), i1.long())


def _batch1(model, spec, row, pos, steps, vl):
    """One row alone: prefill + teacher-forced decode steps, returning the last hidden states of each call.  The batch-1 hook
    decodes with SDPA only (with eager attention its decode mask is sized for the long layout), so the reference runs the same
    weights with SDPA; an eager batch checks its prefill against the eager batch-1 prefill as well."""
    set_one(model, spec, vl)
    attn = model.config._attn_implementation
    eager_prefill = None
    if attn != "sdpa":
        eager_prefill = model(inputs_embeds=row[None], position_ids=pos, use_cache=False).last_hidden_state[0]
        model.config._attn_implementation = "sdpa"
    try:
        outs = []
        res = model(inputs_embeds=row[None], position_ids=pos, use_cache=True)
        outs.append(res.last_hidden_state[0])
        cache = res.past_key_values
        idx = model.merged_token_1d_idx
        for t, (emb, p) in enumerate(steps):
            res = model(inputs_embeds=emb[None], position_ids=p, past_key_values=cache, use_cache=True)
            outs.append(res.last_hidden_state[0])
    finally:
        model.config._attn_implementation = attn
    return outs, idx, eager_prefill


@pytest.mark.parametrize("vl", [False, True], ids=["qwen2", "qwen2vl"])
@pytest.mark.parametrize("attn", ["sdpa", "eager"])
def test_patched_forward_batch_equals_rows_alone(vl, attn):
    pytest.importorskip("transformers")
    C = 32
    if vl:
        pytest.importorskip("transformers.models.qwen2_vl.modeling_qwen2_vl")
        from transformers.models.qwen2_vl.modeling_qwen2_vl import Qwen2VLTextModel as cls
        model, specs = qwen2vl_model(C, attn=attn), VL_ROWS
    else:
        from transformers.models.qwen2.modeling_qwen2 import Qwen2Model as cls
        model, specs = qwen2_model(C, attn=attn), LLAVA_ROWS
    rows = prompt_rows(specs, C, seed=11)
    hs, mask = left_pad(rows, extra_pad=(2,))
    B, L = mask.shape
    lengths = [r.shape[0] for r in rows]
    g = torch.Generator().manual_seed(5)
    step_emb = [torch.randn(B, 1, C, generator=g) for _ in range(3)]
    with installed([cls], merge_fn=O.get_quadtree_features, merge_batch_fn=oracle_batch, pack_fn=pack_merged_batch_ref), \
            torch.inference_mode():
        # batched: what generate passes (left-padded mask, per-row positions), then three decode steps
        set_rows(model, specs, vl)
        pos = mrope_batch(lengths, L) if vl else positions_1d(mask)
        res = model(inputs_embeds=hs, attention_mask=mask, position_ids=pos, use_cache=True)
        outs = [res.last_hidden_state]
        cache = res.past_key_values
        idx_b = model.merged_token_1d_idx
        m = mask
        for t in range(3):
            m = torch.cat([m, torch.ones(B, 1, dtype=m.dtype)], 1)
            last = torch.tensor([n + t for n in lengths]) if not vl else torch.tensor([[mrope_ids(n)[a, -1] + 1 + t for n in lengths]
                                                                                       for a in range(3)])
            p = last[:, None] if not vl else last[:, :, None]
            outs.append(model(inputs_embeds=step_emb[t], attention_mask=m, position_ids=p, past_key_values=cache,
                              use_cache=True).last_hidden_state)
        assert cache.sttm_merged_mask is not None
        Lout = outs[0].shape[1]
        for b, (spec, r) in enumerate(zip(specs, rows)):
            n = lengths[b]
            if vl:
                p1 = mrope_ids(n)[:, None]
                steps = [(step_emb[t][b], torch.stack([mrope_ids(n)[a, -1] + 1 + t for a in range(3)]).view(3, 1, 1)) for t in range(3)]
            else:
                p1 = torch.arange(n)[None]
                steps = [(step_emb[t][b], torch.tensor([[n + t]])) for t in range(3)]
            ref, idx1, eager_prefill = _batch1(model, spec, r, p1, steps, vl)
            n1 = ref[0].shape[0]
            assert Lout >= n1
            if eager_prefill is not None:
                assert torch.allclose(outs[0][b, Lout - n1:], eager_prefill, atol=1e-5)
            assert torch.allclose(outs[0][b, Lout - n1:], ref[0], atol=1e-5), (b, float((outs[0][b, Lout - n1:] - ref[0]).abs().max()))
            assert torch.equal(idx_b[b].long(), idx1.long())
            for t in range(3):
                assert torch.allclose(outs[t + 1][b], ref[t + 1], atol=1e-5), (b, t)


def test_batch1_keeps_its_path():
    """A batch of one with 0-d attributes stores no merged-layout state and returns ONE idx tensor, as before."""
    pytest.importorskip("transformers")
    from transformers.models.qwen2.modeling_qwen2 import Qwen2Model
    model = qwen2_model(32)
    spec = LLAVA_ROWS[0]
    row = prompt_rows([spec], 32)[0]
    with installed([Qwen2Model], merge_fn=O.get_quadtree_features, merge_batch_fn=oracle_batch, pack_fn=pack_merged_batch_ref), \
            torch.inference_mode():
        set_one(model, spec)
        res = model(inputs_embeds=row[None], use_cache=True)
        assert torch.is_tensor(model.merged_token_1d_idx)
        assert getattr(res.past_key_values, "sttm_merged_mask", None) is None
        # the same row as a batch of one with 1-D attributes takes the batched hook and agrees
        set_rows(model, [spec])
        res2 = model(inputs_embeds=row[None], attention_mask=torch.ones(1, row.shape[0], dtype=torch.long), use_cache=True)
        assert isinstance(model.merged_token_1d_idx, list)
        assert torch.allclose(res2.last_hidden_state, res.last_hidden_state, atol=1e-5)


def test_batched_hook_rejects_right_padding_and_bad_attribute_lengths():
    pytest.importorskip("transformers")
    from transformers.models.qwen2.modeling_qwen2 import Qwen2Model
    model = qwen2_model(32)
    rows = prompt_rows(LLAVA_ROWS[:2], 32)
    hs, mask = left_pad(rows)
    with installed([Qwen2Model], merge_fn=O.get_quadtree_features, merge_batch_fn=oracle_batch, pack_fn=pack_merged_batch_ref), \
            torch.inference_mode():
        set_rows(model, LLAVA_ROWS[:2])
        with pytest.raises(ValueError, match="LEFT-padded"):
            model(inputs_embeds=hs, attention_mask=mask.flip(-1), use_cache=False)
        set_rows(model, LLAVA_ROWS)
        with pytest.raises(ValueError, match="entries for a batch of 2"):
            model(inputs_embeds=hs, attention_mask=mask, use_cache=False)


# ---- the C entry point: argument checks (no launch) and the kernels' resources ------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from sttm_amd import _lib
    return _lib.load()


def _call(lib, geom, B=2, C=64, L=100, Lout=100, pos_mode=0, null_feat=False, dtype=0):
    from sttm_amd import _lib
    fake = ctypes.c_void_p(0x100000)                  # never dereferenced: every case below fails validation first
    vp = ctypes.c_void_p * B
    ptrs = vp(*([None if null_feat else fake.value] * B))
    flat = [v for g in geom for v in g]
    return lib.sttm_pack_merged_batch(B, C, dtype, fake, L * C, C, L, ptrs, vp(*([fake.value] * B)), (ctypes.c_int32 * len(flat))(*flat),
                                      Lout, fake, fake, vp(*([fake.value] * B)), pos_mode, None, 0, 0, None, None), _lib


def test_pack_entry_point_validates_its_arguments(lib):
    good = (3, 5, 4 * 16, 10, 4, 4, 4)
    cases = [
        ([good, (0, 5, 4 * 16, 0, 4, 4, 4)], "N' 0"),                        # a video merged to no rows
        ([good, (0, 5, 4 * 16, 65, 4, 4, 4)], "N' 65"),                      # more rows than tokens
        ([good, (0, 5, 60, 10, 4, 4, 4)], "length 60"),                      # length != T * H * W
        ([good, (40, 5, 4 * 16, 10, 4, 4, 4)], "longer than L"),             # runs past the end of the row
        ([good, (-1, 5, 4 * 16, 10, 4, 4, 4)], "pad -1"),
    ]
    for geom, msg in cases:
        rc, _lib = _call(lib, geom)
        assert rc == _lib.ERR_ARG and msg in lib.sttm_last_error().decode(), (geom, lib.sttm_last_error())
    rc, _lib = _call(lib, [good, good], Lout=40)                             # 100 - 3 - 64 + 10 = 43 columns do not fit 40
    assert rc == _lib.ERR_ARG and b"Lout = 40" in lib.sttm_last_error()
    rc, _lib = _call(lib, [good, good], pos_mode=1)
    assert rc == _lib.ERR_ARG and b"pos_in" in lib.sttm_last_error()
    rc, _lib = _call(lib, [good, good], pos_mode=3)
    assert rc == _lib.ERR_ARG
    rc, _lib = _call(lib, [good, good], null_feat=True)
    assert rc == _lib.ERR_ARG and b"null" in lib.sttm_last_error()
    rc, _lib = _call(lib, [good, good], dtype=3)
    assert rc == _lib.ERR_ARG
    assert lib.sttm_abi_version() == 8


def test_pack_kernels_use_no_scratch():
    from tests.test_kernel_resources import LLVM, _kernels_of
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(f"{LLVM}/{tool}"):
            pytest.skip(f"{tool} not available")
    k = _kernels_of(LIB)
    names = [f"_ZN4sttm13k_pack_mergedILi{w}EEEvNS_8PackArgsE" for w in (16, 8, 4, 2)]
    missing = [n for n in names if n not in k]
    assert not missing, f"pack kernels missing from the library: {missing}"
    spilled = {n: k[n] for n in names if k[n][0] != 0}
    assert not spilled, f"pack kernels with scratch (bytes per lane, VGPRs): {spilled}"
