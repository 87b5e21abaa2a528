#!/usr/bin/env python3
"""Generate the off-distribution golden vectors tests/golden/od_*.npz by RUNNING THE REFERENCE.

Like make_golden.py this runs only where the reference checkout is available (STTM_REFERENCE, default /root/reference): it imports
the reference's own `token_merging_utils.quadtree_interface.get_quadtree_features` (pure PyTorch, CPU) and records its outputs on the
degenerate clips of tests/_offdist.py -- all-zero tokens / frames / videos, duplicated and static frames, a constant video, NaN and
Inf elements, power-of-two scalings down to the eps clamp and up to fp32 norm overflow, and clips in which everything merges.
Only data is written.  Nothing under tests/ reads the reference at test time.

The fixtures have make_golden.py's format (x_thwc, feat, npatch, tlbr, meta).  Clips of 32 and more frames do not fit a committed
file: for those the fixture holds the outputs and the SHA-256 of the input, which tests/_offdist.load_od rebuilds and verifies.

The octree baseline's degenerate clips (odoct_*.npz) come from the reference's `get_octree_features` the same way.

    python tests/golden/make_golden_offdist.py            # rewrites tests/golden/od_*.npz and odoct_*.npz
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

from tests import _offdist as D                                           # noqa: E402
from token_merging_utils.quadtree_interface import get_quadtree_features  # noqa: E402  (reference)
from token_merging_utils.octree_utils import get_octree_features           # noqa: E402  (reference)


def to_np(t):
    if t.element_size() == 2:
        return t.contiguous().view(torch.int16).numpy()
    return t.contiguous().numpy()


def main():
    torch.set_num_threads(8)
    for name, (_, kw, dtypes, store_input) in D.DEGENERATE.items():
        for dname in dtypes:
            fid = f"od_{name}_{D.SHORT[dname]}"
            x = D.build_degenerate(name, D.DTYPES[dname])
            args = dict(kw)
            thr = args.pop("threshold")
            feat, npatch, tlbr = get_quadtree_features(x, thr, **args)[:3]
            T, C, H, W = x.shape
            meta = dict(name=fid, case=name, fn="quadtree", dtype=dname, T=T, C=C, H=H, W=W, kw=kw, x_sha256=D.digest(x))
            arrays = dict(feat=to_np(feat), npatch=to_np(npatch), tlbr=to_np(tlbr), meta=json.dumps(meta))
            if store_input:
                mem = x.permute(0, 2, 3, 1)
                assert mem.is_contiguous()
                arrays["x_thwc"] = to_np(mem)
            path = os.path.join(HERE, fid + ".npz")
            np.savez_compressed(path, **arrays)
            f = feat.float()
            print(f"{fid}: N'={feat.shape[0]} of {T * H * W}, largest group {int(npatch.max())} patches, NaN {int(torch.isnan(f).sum())}, "
                  f"Inf {int(torch.isinf(f).sum())}, {os.path.getsize(path) // 1024} KB")
            assert os.path.getsize(path) < 512 * 1024, fid
    for kind in D.OCTREE_KINDS:                                   # the octree baseline decides with the same test: odoct_*.npz
        x = D.build_octree_degenerate(kind)
        feat = get_octree_features(x, D.OCTREE_THR, D.OCTREE_ROOT)
        path = os.path.join(HERE, f"odoct_{kind}.npz")
        meta = dict(name=f"odoct_{kind}", fn="octree", dtype="float32", thr=D.OCTREE_THR, root=D.OCTREE_ROOT)
        np.savez_compressed(path, meta=json.dumps(meta), x_thwc=to_np(x.permute(0, 2, 3, 1)), feat=to_np(feat))
        print(f"odoct_{kind}: {feat.shape[0]} of {x.shape[0] * 64} tokens, NaN {int(torch.isnan(feat).sum())}, Inf {int(torch.isinf(feat).sum())}, "
              f"{os.path.getsize(path) // 1024} KB")
        assert os.path.getsize(path) < 512 * 1024, kind


if __name__ == "__main__":
    main()
