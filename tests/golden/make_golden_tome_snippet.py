"""Golden vectors of per-frame / per-snippet ToMe: the REFERENCE's own `tome_per_video` (tome_token_merger.py:133-152) on CPU,
called once per snippet of S frames, ids offset to the whole clip, results concatenated in time order.

    STTM_REFERENCE_DIR=<checkout of the reference> python tests/golden/make_golden_tome_snippet.py

The reference's `tome_per_frame` keeps a [1, n, 1] token index next to [T, n, C] features and raises for T > 1; its building
blocks (`bipartite_soft_matching`, `merge_wavg`) are batched, though.  For the S = 1 cases this script also runs them on the
[T, n, C] batch with the index repaired to [T, n, 1] and asserts the same bits as the per-snippet calls.
Inputs are only taken where they hold no open decision (tests/_tome_snippet_ref.py): a seed that fails the condition with the
installed torch is skipped and the next one tried; the seed used is in the fixture's meta.
Only inputs, outputs and meta are stored: no reference code.
"""
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.environ["STTM_REFERENCE_DIR"])

from sttm_amd.synth import synth_video                                                                  # noqa: E402
from tests._tome_snippet_ref import open_snippets, snippet_ranges                                      # noqa: E402
from token_merging_utils.tome_token_merger import bipartite_soft_matching, merge_wavg, tome_per_video  # noqa: E402  (reference)

CASES = [
    dict(name="tsn_s1_050", T=4, C=64, H=14, W=14, seed=300, S=1, ratio=0.50, n_head=1, dtype="float32"),
    dict(name="tsn_s3_085_tail", T=10, C=64, H=14, W=14, seed=300, S=3, ratio=0.85, n_head=1, dtype="float32"),
    dict(name="tsn_s1_070_odd", T=5, C=64, H=7, W=7, seed=300, S=1, ratio=0.70, n_head=1, dtype="float32"),
    dict(name="tsn_s2_070_h4", T=7, C=64, H=14, W=14, seed=301, S=2, ratio=0.70, n_head=4, dtype="float32"),
    dict(name="tsn16_bf16_s1_070", T=4, C=64, H=14, W=14, seed=400, S=1, ratio=0.70, n_head=1, dtype="bfloat16"),
    dict(name="tsn16_bf16_s2_085", T=6, C=128, H=14, W=14, seed=406, S=2, ratio=0.85, n_head=1, dtype="bfloat16"),
    dict(name="tsn16_bf16_s1_030", T=4, C=64, H=14, W=14, seed=408, S=1, ratio=0.30, n_head=1, dtype="bfloat16"),
    dict(name="tsn16_bf16_s1_060_odd", T=5, C=64, H=7, W=7, seed=400, S=1, ratio=0.60, n_head=1, dtype="bfloat16"),
    dict(name="tsn16_f16_s1_070", T=4, C=64, H=14, W=14, seed=400, S=1, ratio=0.70, n_head=1, dtype="float16"),
    dict(name="tsn16_f16_s2_085", T=6, C=128, H=14, W=14, seed=400, S=2, ratio=0.85, n_head=1, dtype="float16"),
]


def to_np(t):
    t = t.contiguous()
    return t.view(torch.int16).numpy() if t.dtype in (torch.bfloat16, torch.float16) else t.numpy()


def per_snippet(x, S, ratio, n_head):
    hw = x.shape[2] * x.shape[3]
    feats, ids = [], []
    for t0, t1 in snippet_ranges(x.shape[0], S):
        f, i = tome_per_video(x[t0:t1], ratio, n_head)
        feats.append(f)
        ids.append(i + t0 * hw)
    return torch.cat(feats), torch.cat(ids)


def per_frame_repaired(x, ratio, n_head):
    """The reference's batched matching and merge on [T, n, C] with one token index per frame."""
    T, C, H, W = x.shape
    n = H * W
    tokens = x.permute(0, 2, 3, 1).reshape(T, n, C)
    index = torch.arange(n).reshape(1, n, 1).repeat(T, 1, 1)
    target, size, done = math.ceil(n * (1 - ratio)), None, False
    while not done or tokens.shape[1] > target:
        done = True
        cur = tokens.shape[1]
        merge, _ = bipartite_soft_matching(tokens.reshape(T, cur, n_head, C // n_head).mean(2), cur - target)
        tokens, index, size = merge_wavg(merge, tokens, index, size)
    ids = index.reshape(T, -1) + torch.arange(T).reshape(T, 1) * n
    return tokens.reshape(-1, C), ids.reshape(-1)


def main():
    for case in CASES:
        dt = getattr(torch, case["dtype"])
        for seed in range(case["seed"], case["seed"] + 64):
            x = synth_video(case["T"], case["C"], case["H"], case["W"], seed=seed, dtype=dt)
            if not open_snippets(x, case["ratio"], case["S"], case["n_head"]):
                break
        else:
            raise SystemExit(f"{case['name']}: no seed without an open decision")
        case = dict(case, seed=seed)
        feat, idx = per_snippet(x, case["S"], case["ratio"], case["n_head"])
        assert feat.dtype == dt and idx.dtype == torch.int64
        if case["S"] == 1:
            f2, i2 = per_frame_repaired(x, case["ratio"], case["n_head"])
            assert torch.equal(i2, idx) and torch.equal(to_np_t(f2), to_np_t(feat)), f"{case['name']}: repaired tome_per_frame differs"
        path = os.path.join(HERE, case["name"] + ".npz")
        np.savez_compressed(path, x_thwc=to_np(x.permute(0, 2, 3, 1)), feat=to_np(feat), idx=to_np(idx),
                            meta=json.dumps(dict(case, fn="tome_snippet", torch=torch.__version__,
                                                 torch_parallel=torch.__config__.parallel_info().splitlines()[:4],
                                                 torch_has_fbgemm="USE_FBGEMM=ON" in torch.__config__.show())))
        print(case["name"], "seed", seed, tuple(feat.shape), os.path.getsize(path), "bytes")


def to_np_t(t):
    return torch.from_numpy(to_np(t).copy())


if __name__ == "__main__":
    main()
