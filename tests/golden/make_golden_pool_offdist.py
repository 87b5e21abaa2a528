#!/usr/bin/env python3
"""Off-distribution vectors for the upstream 2-D pooling step, made by RUNNING THE REFERENCE's `LlavaMetaForCausalLM.get_2dPool`
(llava/model/llava_arch.py:173-198) in the build container (CPU), like make_golden_pool.py: that ONE method is compiled out of the
reference file at generation time (nothing is copied into the repo).  The inputs are tests/_pool_offdist.build's: NaN / +Inf / -Inf
elements in the first, an interior and the last window and in the dropped row / column, a zero frame, scalings by 2^62 and 2^-70.
One file per (kind, shape, dtype) with the reference's output in all three modes.  Only data is written.

    python tests/golden/make_golden_pool_offdist.py        # rewrites tests/golden/poolod_*.npz
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from make_golden_pool import reference_get_2dpool, to_np                 # noqa: E402
from tests import _pool_offdist as PD                                    # noqa: E402


def main():
    fn = reference_get_2dpool()
    for case in PD.cases():
        kind, side, stride, dname = case
        x = PD.build(kind, side, stride, PD.DTYPES[dname])
        arrays = dict(x=to_np(x))
        for mode in PD.MODES:
            me = types.SimpleNamespace(config=types.SimpleNamespace(mm_spatial_pool_mode=mode),
                                       get_vision_tower=lambda side=side: types.SimpleNamespace(num_patches_per_side=side))
            arrays["y_" + mode] = to_np(fn(me, x.clone(), stride=stride))
        meta = dict(name=PD.fixture_name(case), fn="pool2d", kind=kind, side=side, stride=stride, dtype=dname, T=PD.T, C=PD.C)
        path = os.path.join(HERE, PD.fixture_name(case) + ".npz")
        np.savez_compressed(path, meta=json.dumps(meta), **arrays)
        print(PD.fixture_name(case), {m: tuple(arrays["y_" + m].shape) for m in PD.MODES}, os.path.getsize(path) // 1024, "KB")
        assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    main()
