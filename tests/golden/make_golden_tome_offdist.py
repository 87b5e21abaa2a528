#!/usr/bin/env python3
"""Generate the off-distribution ToMe golden vectors tests/golden/tomeod_*.npz by RUNNING THE REFERENCE.

Like the other make_golden_*.py this runs only where the reference checkout is available (STTM_REFERENCE, default /root/reference): it
imports the reference's own `token_merging_utils.tome_interface.get_tome_features` (pure PyTorch, CPU) and records its outputs on the
families of tests/_tome_offdist.py -- all-zero tokens / frames / videos, NaN and Inf elements on either side of the bipartite split,
constant and duplicated clips, norms that underflow and overflow, float16 merge sums past 65 504, a NaN in one head.  Only data is
written.  Nothing under tests/ reads the reference at test time.

One file per family and dtype: the input (x_thwc), and feat_rXXX / idx_rXXX for every ratio of the family.

A clip is committed only if the reference alone is well determined on it (tests/_tome_offdist.well_determined: the same loop with
float64 scores takes the same node_idx and keeps the same ids); otherwise the next seed is tried and the rejection is printed -- the
table SEEDS of tests/_tome_offdist.py and profiles/tome_offdist.md record them.

    python tests/golden/make_golden_tome_offdist.py            # rewrites tests/golden/tomeod_*.npz
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("STTM_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, REF)

from tests import _tome_offdist as D                                         # noqa: E402
from tests._offdist import DTYPES, SHORT                                     # noqa: E402
from token_merging_utils.tome_interface import get_tome_features           # noqa: E402  (reference)

MAX_SEEDS = 8


def to_np(t):
    t = t.contiguous()
    return t.view(torch.int16).numpy() if t.element_size() == 2 else t.numpy()


def main():
    torch.set_num_threads(8)
    for name, (_, shape, n_head, dtypes, ratios) in D.FAMILIES.items():
        for dname in dtypes:
            fid = f"tomeod_{name}_{SHORT[dname]}"
            first = D.seed_of(name, dname)
            for seed in range(first, first + MAX_SEEDS):
                x = D.build(name, dname, seed)
                why = [(r, D.well_determined(x, r, n_head)) for r in ratios]
                bad = [(r, w) for r, (ok, w) in why if not ok]
                if not bad:
                    break
                print(f"{fid}: seed {seed} rejected: " + "; ".join(f"ratio {r}: {w}" for r, w in bad))
            else:
                raise SystemExit(f"{fid}: no seed in {first}..{first + MAX_SEEDS - 1} gives a well-determined clip")
            if seed != first:
                print(f"{fid}: put ({name!r}, {dname!r}): {seed} into tests/_tome_offdist.SEEDS")
            T, C, H, W = shape
            meta = dict(name=fid, case=name, fn="tome", dtype=dname, T=T, C=C, H=H, W=W, seed=seed, n_head=n_head, ratios=list(ratios),
                        torch=torch.__version__)
            arrays = dict(x_thwc=to_np(x.permute(0, 2, 3, 1)), meta=json.dumps(meta))
            notes = []
            for r in ratios:
                feat, idx = get_tome_features(x, r, "video", n_head)
                assert feat.dtype == DTYPES[dname] and idx.dtype == torch.int64
                arrays["feat_" + D.ratio_key(r)], arrays["idx_" + D.ratio_key(r)] = to_np(feat), to_np(idx)
                f = feat.float()
                notes.append(f"r={r}: {feat.shape[0]} kept, NaN {int(torch.isnan(f).sum())}, Inf {int(torch.isinf(f).sum())}, ids {idx[:4].tolist()}")
            path = os.path.join(HERE, fid + ".npz")
            np.savez_compressed(path, **arrays)
            print(f"{fid}: seed {seed}; " + "; ".join(notes) + f"; {os.path.getsize(path) // 1024} KB")
            assert os.path.getsize(path) < 128 * 1024, fid


if __name__ == "__main__":
    main()
