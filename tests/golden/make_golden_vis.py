#!/usr/bin/env python3
"""Generate tests/golden/vis_*.npz by RUNNING THE REFERENCE with vis_flag=True.

Runs only in the build container, where the reference checkout is mounted read-only (STTM_REFERENCE, default /root/reference).
It imports the reference's own `token_merging_utils` (pure PyTorch, CPU) and records, for seeded inputs, the outputs of
`get_quadtree_features(..., vis_flag=True)`: the three tensors and `node_metadata`, flattened as keys [G], counts [G] and
boxes [sum(counts), 5].  Only data is written; nothing under tests/ reads the reference at test time.  Every case is also
checked against tests/_token_map_ref.py's derivation from the oracle before it is written.

    python tests/golden/make_golden_vis.py
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

from sttm_amd.synth import synth_video                                    # noqa: E402
from tests._token_map_ref import ref_token_maps                           # noqa: E402
from token_merging_utils.quadtree_interface import get_quadtree_features  # noqa: E402  (reference)

CASES = [
    dict(name="vis_14_r1", T=4, C=32, H=14, W=14, seed=500, root_level=1),
    dict(name="vis_13x24_r1", T=3, C=16, H=13, W=24, seed=501, root_level=1),          # mixed parity
    dict(name="vis_27_r0", T=2, C=16, H=27, W=27, seed=502, root_level=0),             # 5 levels, groups of more than 10 members
    dict(name="vis_3x5_r0", T=4, C=16, H=3, W=5, seed=503, root_level=0),
    dict(name="vis_5x5_rm1", T=3, C=16, H=5, W=5, seed=504, root_level=-1),            # no pyramid
    dict(name="vis_14_r1_w", T=4, C=32, H=14, W=14, seed=505, root_level=1, weighted_avg=True),
]


def main():
    torch.set_num_threads(8)
    for case in CASES:
        case = dict(dict(threshold=0.85, temporal_thresh=0.55, weighted_avg=False, dtype="float32"), **case)
        x = synth_video(case["T"], case["C"], case["H"], case["W"], seed=case["seed"])
        feat, npatch, tlbr, md = get_quadtree_features(x, case["threshold"], case["temporal_thresh"], case["root_level"],
                                                       weighted_avg=case["weighted_avg"], vis_flag=True)
        keys = list(md.keys())
        assert keys == sorted(keys)
        counts = [len(md[k]) for k in keys]
        boxes = [b for k in keys for b in md[k]]
        ours = ref_token_maps(x, case["threshold"], case["temporal_thresh"], case["root_level"], case["weighted_avg"])
        assert ours["node_metadata"] == md and list(ours["node_metadata"]) == keys, case["name"]
        mem = x.permute(0, 2, 3, 1)
        assert mem.is_contiguous()
        np.savez_compressed(os.path.join(HERE, case["name"] + ".npz"), x_thwc=mem.numpy(), feat=feat.contiguous().numpy(),
                            npatch=npatch.numpy(), tlbr=tlbr.numpy(), keys=np.asarray(keys, dtype=np.int32),
                            counts=np.asarray(counts, dtype=np.int32), boxes=np.asarray(boxes, dtype=np.int32).reshape(-1, 5),
                            meta=json.dumps(dict(case, fn="quadtree_vis")))
        print(case["name"], dict(N=int(feat.shape[0]), nodes=len(boxes), groups=len(keys), largest=max(counts)))


if __name__ == "__main__":
    main()
