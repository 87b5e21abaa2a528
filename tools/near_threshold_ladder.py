#!/usr/bin/env python3
"""In-band flip rates of the near-threshold ladders (tests/_offdist.py), per path and per rung: what is recorded, not asserted.

For each ladder video the band is eps = 2 * max |sim_oracle_fp32 - sim_float64|.  Outside it the device, the oracle and float64
agree (tests/test_hip_offdist.py asserts that; this tool stops if it does not hold).  Inside it a decision may legitimately depend
on the summation order; this tool counts, among the decisions inside the band, how often the device differs from the oracle, the
device from float64 and the oracle from float64, split by the rung |delta| the decision was built at.

One process on one device does the work: this command starts it as a child and ends it (SIGKILL) when the whole run exceeds
RUN_LIMIT_S, which also ends a kernel that hangs inside the runtime.  Inside the child every step has its own limit (SIGALRM, which
Python serves between two calls); the first step that fails or overruns ends the run.

    python tools/near_threshold_ladder.py > profiles/near_threshold_ladder.md
"""
import os
import signal
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from sttm_amd import _lib, get_quadtree_features                                        # noqa: E402
from sttm_amd.quadtree_interface import get_quadtree_features_batch, temporal_merge_nodes   # noqa: E402
from tests import _offdist as D                                                         # noqa: E402

STEP_LIMIT_S = 60
RUN_LIMIT_S = 300
DEV = "cuda:0"
RESET = dict(k1_split=0, pairs_var=0, col_walk=0, col_frames=8, col_cap=0, col_pb=0)


def plain(lad, **extra):
    return lad.decode(get_quadtree_features(lad.x.to(DEV), lad.thr, **lad.kwargs(**extra))[2])


def switched(**opts):
    def run(lad):
        try:
            _lib.configure(**opts)
            out = plain(lad)
            torch.cuda.synchronize()
        finally:
            _lib.configure(**RESET)
        return out
    return run


def nodes(lad):
    T, H, W, C = lad.T, lad.H, lad.W, lad.C
    t, y, x = torch.meshgrid(torch.arange(T), torch.arange(H), torch.arange(W), indexing="ij")
    tlbr = torch.stack([t, y, x, y + 1, x + 1], dim=-1).reshape(-1, 5).to(torch.int32)
    feats = lad.x.permute(0, 2, 3, 1).reshape(T * H * W, C)
    return lad.decode(temporal_merge_nodes(feats.to(DEV), tlbr.to(DEV), lad.tthr, grid=(T, H, W), root_level=1)[2])


def batch(lads):
    outs = get_quadtree_features_batch([l.x.to(DEV) for l in lads], lads[0].thr, **lads[0].kwargs())
    return [l.decode(o[2]) for l, o in zip(lads, outs)]


# (path, ladder specs, runner of one ladder) -- the paths of tests/test_hip_offdist.py
PATHS = [
    ("default", D.DEFAULT_LADDERS, plain),
    ("col_walk=2", D.COLWALK_LADDERS, switched(col_walk=2)),
    ("pairs_var=9", D.COLWALK_LADDERS, switched(pairs_var=9)),
    ("head_dim=128", D.HEAD_LADDERS, plain),
    ("slow_ver", D.SLOW_LADDERS, lambda lad: plain(lad, slow_ver=True)),
    ("temporal_merge_nodes", D.NODES_LADDERS, nodes),
    ("channel-tiled rows", D.WIDE_LADDERS, plain),
    ("6-level tree, split form", D.DEEP_LADDERS, plain),
    ("6-level tree, one workgroup", D.DEEP_LADDERS, switched(k1_split=-1)),
]


def _overrun(signum, frame):
    raise TimeoutError(f"a step ran longer than {STEP_LIMIT_S} s")


def row(path, spec, lad, got):
    lad.assert_outside_band(got, f"{path} {D.ladder_id(spec)}")
    cells = []
    total = [0, 0, 0, 0]
    for r in D.RUNGS:
        n, a = lad.flips_by_rung(got, lad.want32)[r]
        _, b = lad.flips_by_rung(got, lad.want64)[r]
        _, c = lad.flips_by_rung(lad.want32, lad.want64)[r]
        cells.append(f"{n}: {a}/{b}/{c}")
        total = [u + v for u, v in zip(total, (n, a, b, c))]
    n, a, b, c = total
    rate = f"{100.0 * a / n:.1f} %" if n else "-"
    print(f"| {path} | {D.ladder_id(spec)} | {lad.eps:.2e} | {lad.outside.numel()} | " + " | ".join(cells) + f" | {n}: {a}/{b}/{c} | {rate} |", flush=True)


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    signal.signal(signal.SIGALRM, _overrun)
    print("# Near-threshold ladders: decisions inside the band, per path and rung\n")
    print(f"Library build {_lib.build_tag()}, {torch.cuda.get_device_name(0)}, torch {torch.__version__}; `python tools/near_threshold_ladder.py`.\n")
    print("A cell reads `decisions inside the band: device != oracle / device != float64 / oracle != float64`.  eps = 2 x the largest\n"
          "error of the oracle's fp32 similarity against float64 over the video's ladder decisions.  Outside the band all three agree on\n"
          "every decision of every row (asserted).  Rungs above 1e-7 have decisions inside the band only for 16-bit inputs.\n"
          "Spatial ladders of 256 and more channels run with the temporal stage on (it keeps no pair): only then do `col_walk` and\n"
          "`pairs_var` select other kernels.  The column walk sums in the default path's order, so its rows repeat the default figures.\n")
    print("| path | ladder | eps | decisions | " + " | ".join(f"rung {r:g}" for r in D.RUNGS) + " | all rungs | device != oracle in band |")
    print("|---|---|---|---|" + "---|" * len(D.RUNGS) + "---|---|")
    for path, specs, run in PATHS:
        for spec in specs:
            lad = D.ladder(*spec)
            signal.alarm(STEP_LIMIT_S)
            got = run(lad)
            signal.alarm(0)
            row(path, spec, lad, got)
    for name, specs, col_walk in (("batch, temporal", D.BATCH_LADDERS, 0), ("batch, spatial", D.BATCH_SPATIAL_LADDERS, 0),
                                  ("batch, col_walk=1, temporal", D.BATCH_LADDERS, 1), ("batch, col_walk=1, spatial", D.BATCH_SPATIAL_LADDERS, 1)):
        lads = [D.ladder(*s) for s in specs]
        signal.alarm(STEP_LIMIT_S)
        try:
            _lib.configure(col_walk=col_walk)
            gots = batch(lads)
            torch.cuda.synchronize()
        finally:
            _lib.configure(**RESET)
        signal.alarm(0)
        for spec, lad, got in zip(specs, lads, gots):
            row(f"{name} T={lad.T}", spec, lad, got)


if __name__ == "__main__":
    if "--child" in sys.argv:
        main()
    else:
        try:
            sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], timeout=RUN_LIMIT_S).returncode)
        except subprocess.TimeoutExpired:
            sys.exit(f"the run exceeded {RUN_LIMIT_S} s and was ended")
