#!/usr/bin/env python3
"""Degenerate clips for the octree baseline on ODD cube sides (7: 7-4-2, 5: 5-3-2), made by RUNNING THE REFERENCE's
`get_octree_features` (token_merging_utils/octree_utils.py:293-386) in the build container (CPU, float32).  On an odd level a parent
with fewer than 8 children compares its missing slots with child cell (0, 0, 0) of the cube: a constant or static video makes such
cells stop, a zero / NaN / Inf origin leaf changes every alias comparison of its cube.  Only data is written.

One file per (kind, side): the input (two cubes plus a remainder frame) and the reference's rows at every threshold of
tests/_octree_offdist.deg_thresholds(kind).

    python tests/golden/make_golden_octree_offdist.py        # rewrites tests/golden/odo_*.npz
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

from tests import _octree_offdist as X                                   # noqa: E402
from token_merging_utils.octree_utils import get_octree_features        # noqa: E402  (reference)


def main():
    for side in X.DEG_SIDES:
        for kind in X.DEG_KINDS:
            x = X.build_deg(kind, side)
            thrs = list(X.deg_thresholds(kind))
            arrays = dict(x_thwc=x.permute(0, 2, 3, 1).contiguous().numpy())
            counts = []
            for i, thr in enumerate(thrs):
                feat = get_octree_features(x.clone(), thr, 0)
                arrays[f"feat{i}"] = feat.contiguous().numpy()
                counts.append(int(feat.shape[0]))
            meta = dict(name=X.deg_file(kind, side), fn="octree", dtype="float32", kind=kind, side=side, root=0, thresholds=thrs, rows=counts)
            path = os.path.join(HERE, X.deg_file(kind, side) + ".npz")
            np.savez_compressed(path, meta=json.dumps(meta), **arrays)
            print(f"{X.deg_file(kind, side)}: rows {dict(zip(thrs, counts))} of {x.shape[0] * side * side}, {os.path.getsize(path) // 1024} KB")
            assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main()
