"""DyCoke stage 2 on the device: the decode-time half of the reference's "dycoke" pattern
(token_merging_monkey_patch/dycoke_attn_monkey_patch.py), batch size 1, one query token per step.

    decode_attn_scores         head-mean softmax row of the current token at layer dycoke_l - 1 (:80, :410-411), float32
    select_keep                prefix ++ the num_keep largest scores of the visual window ++ tail (:62-77), an int32 tensor on the device
    gathered_decode_attention  attention of the one query over the kept rows of the cache, read in place (:54-60)

HIP kernels in csrc/dycoke_decode.hip; nothing here synchronises the stream, and the keep list never visits the host.  Ties between
equal scores go to the smaller index (`torch.topk` leaves them unspecified), and the kept window indices are in ascending order.
"""
import torch

from . import _lib

_ws_cache = _lib.BoundedCache(8)      # (device, stream) -> scratch; bounded, see _lib.BoundedCache
_CODES = {torch.float32: _lib.STTM_F32, torch.bfloat16: _lib.STTM_BF16, torch.float16: _lib.STTM_F16}
HEAD_DIMS = (64, 128)


def num_keep_of(n0, dycoke_p):
    return int(n0 * (1 - dycoke_p))                                          # :66


def keep_geometry(Lk, start, n0, num_keep):
    """(window length, tail length, n_keep) of a decode step; RuntimeError where the reference's topk raises (:69)."""
    window = min(start + n0, Lk) - start
    if num_keep > window:
        raise RuntimeError(f"selected index k out of range: num_keep {num_keep} exceeds the window of {window} scores "
                           f"[{start}, {min(start + n0, Lk)})")
    tail = max(Lk - start - n0, 0)
    return window, tail, start + num_keep + tail


def _check(q, k, what):
    if not (q.is_cuda and k.is_cuda):
        raise RuntimeError(f"sttm_amd runs on the GPU only: {what} needs CUDA (ROCm) tensors; there is no CPU fallback")
    if q.dim() != 4 or k.dim() != 4 or q.shape[0] != 1 or k.shape[0] != 1:
        raise NotImplementedError(f"{what}: batch size {q.shape[0]} (DyCoke stage 2 is built for batch size 1)")
    if q.shape[2] != 1:
        raise ValueError(f"{what}: one query token per decode step, got {q.shape[2]}")
    if q.dtype not in _CODES or k.dtype != q.dtype:
        raise NotImplementedError(f"{what}: dtype {q.dtype} / {k.dtype} is not supported (float32, bfloat16, float16, the same for all)")
    if q.shape[3] not in HEAD_DIMS or k.shape[3] != q.shape[3]:
        raise NotImplementedError(f"{what}: head dimension {q.shape[3]} is not built (64 and 128 are)")
    if q.shape[1] % k.shape[1]:
        raise ValueError(f"{what}: {q.shape[1]} query heads over {k.shape[1]} key / value heads")


def _rows16(t):
    """The tensor, or a contiguous copy when a row would not start on a 16-byte boundary."""
    eb = t.element_size()
    if t.stride(-1) != 1 or any((s * eb) % 16 for s in t.stride()[1:3]):
        t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone()              # contiguous already, but its storage starts off a 16-byte boundary: `.contiguous()` returns it as it is
    return t


def _workspace(dev, stream, nbytes):
    key = (dev, stream.cuda_stream)
    nbytes = (nbytes + (1 << 20)) & ~((1 << 20) - 1)         # the cache grows by a row per step: reallocate once in thousands of steps
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _ws_cache[key] = ws
    return ws


def decode_attn_scores(query, key, scaling):
    """query [1, Hq, 1, D], key [1, Hkv, Lk, D] (the cache layer, any strides) -> score [Lk] float32."""
    _check(query, key, "decode_attn_scores")
    lib = _lib.load()
    q, k = _rows16(query), _rows16(key)
    Hq, D, Hkv, Lk = q.shape[1], q.shape[3], k.shape[1], k.shape[2]
    dev = q.device
    nbytes = lib.sttm_decode_workspace_bytes(Hq, Lk, 0)
    if nbytes == 0:
        raise NotImplementedError(_lib.last_error())
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        ws = _workspace(dev, stream, nbytes)
        score = torch.empty(Lk, dtype=torch.float32, device=dev)
        rc = lib.sttm_decode_attn_scores(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), k.stride(2), Hq, Hkv, Lk, D, _CODES[q.dtype],
                                         float(scaling), ws.data_ptr(), ws.numel(), score.data_ptr(), stream.cuda_stream)
    _lib.raise_for(rc)
    return score


def select_keep(score, start, n0, num_keep):
    """score [Lk] float32 on the device -> keep [start + num_keep + tail] int32 on the device (see the module docstring)."""
    if not score.is_cuda:
        raise RuntimeError("sttm_amd runs on the GPU only: select_keep needs a CUDA (ROCm) tensor; there is no CPU fallback")
    if score.dim() != 1 or score.dtype != torch.float32:
        raise ValueError("select_keep: the scores are a 1-D float32 tensor")
    Lk = score.numel()
    _, _, n_keep = keep_geometry(Lk, start, n0, num_keep)                      # raises before any launch
    if n_keep == 0:
        return torch.empty(0, dtype=torch.int32, device=score.device)
    lib = _lib.load()
    s = score.contiguous()
    dev = s.device
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        keep = torch.empty(n_keep, dtype=torch.int32, device=dev)
        rc = lib.sttm_decode_select_keep(s.data_ptr(), Lk, int(start), int(n0), int(num_keep), keep.data_ptr(), n_keep, stream.cuda_stream)
    _lib.raise_for(rc)
    return keep


def gathered_decode_attention(query, key, value, keep, scaling):
    """query [1, Hq, 1, D], key / value [1, Hkv, Lk, D], keep [n] int32 -> [1, 1, Hq, D] in the model dtype (the layout attention
    functions of transformers return)."""
    _check(query, key, "gathered_decode_attention")
    _check(query, value, "gathered_decode_attention")
    if not keep.is_cuda or keep.dtype != torch.int32 or keep.dim() != 1:
        raise ValueError("gathered_decode_attention: the keep list is a 1-D int32 tensor on the device")
    lib = _lib.load()
    q, k, v, kp = _rows16(query), _rows16(key), _rows16(value), keep.contiguous()
    Hq, D, Hkv, Lk = q.shape[1], q.shape[3], k.shape[1], k.shape[2]
    dev = q.device
    nbytes = lib.sttm_decode_workspace_bytes(Hq, Lk, kp.numel())
    if nbytes == 0:
        raise NotImplementedError(_lib.last_error())
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        ws = _workspace(dev, stream, nbytes)
        out = torch.empty((1, 1, Hq, D), dtype=q.dtype, device=dev)
        rc = lib.sttm_decode_attn_gathered(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), k.stride(2), v.data_ptr(), v.stride(1),
                                           v.stride(2), Hq, Hkv, Lk, D, _CODES[q.dtype], float(scaling), kp.data_ptr(), kp.numel(),
                                           ws.data_ptr(), ws.numel(), out.data_ptr(), stream.cuda_stream)
    _lib.raise_for(rc)
    return out
