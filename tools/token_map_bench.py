"""What the token map costs on the one-call path, and what unmerge_tokens reaches, on the GPU.

    python tools/token_map_bench.py [--out profiles/token_map_bench.json] [--window 0.5] [--rounds 5]

Shapes: the headline (T = 128, 14 x 14, fp32 C = 1024, synth-v1, 0.85 / 0.55, root_level 1) and the hook shape (bf16 C = 3584).
  comparison 1   quadtree_merge_raw(...) against quadtree_merge_raw(..., want_map=True), microseconds per call (the host's wait for
                 N' included: it is part of the call).  The difference is the map's cost: two small launches.
  unmerge        unmerge_tokens(features, token_to_out, out=dest) (torch.index_select, the int64 copy of the map counted):
                 microseconds, bytes/s over the algorithmic bytes (T*H*W*C*eb written + N'*C*eb read) and the share of the 8 TB/s
                 peak.  The figure a gather kernel of the library's own would have to beat by more than this leg's spread.
One process, everything warmed; the two legs of a comparison alternate, window after window, every window at least --window
seconds of back-to-back calls ending in a synchronise; --rounds windows per leg.  A leg's figure is the median of its windows, its
spread (max - min) / median.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

PEAK_BYTES_PER_S = 8e12


def _window_us(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / calls


def _calibrate(fn, seconds):
    for _ in range(5):
        fn()
    return max(5, math.ceil(seconds * 1e6 / _window_us(fn, 5)))


def _compare(legs, seconds, rounds):
    """legs: {name: fn}.  Alternates the legs window by window; returns {name: {us, spread, windows_us, calls_per_window}}."""
    calls = {k: _calibrate(fn, seconds) for k, fn in legs.items()}
    wins = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            wins[k].append(_window_us(fn, calls[k]))
    out = {}
    for k, w in wins.items():
        med = statistics.median(w)
        out[k] = dict(us=round(med, 3), spread=round((max(w) - min(w)) / med, 4), windows_us=[round(v, 3) for v in w],
                      calls_per_window=calls[k])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "token_map_bench.json"))
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=128)
    a = ap.parse_args()
    import sttm_amd
    from sttm_amd import _lib
    from sttm_amd.quadtree_interface import quadtree_merge_raw
    from sttm_amd.synth import synth_video
    dev = torch.device("cuda:0")
    results = []
    for dtype, C in ((torch.float32, 1024), (torch.bfloat16, 3584)):
        T, H, W = a.frames, 14, 14
        x = synth_video(T, C, H, W, seed=0, dtype=dtype).to(dev)
        args = (0.85, 0.55, 1, False, None)
        feat, npatch, tlbr, t2o, t2n = sttm_amd.get_quadtree_features_with_map(x, 0.85, 0.55, 1, False)
        n_out, eb = feat.shape[0], feat.element_size()
        assert torch.equal(torch.bincount(t2o.flatten().long(), minlength=n_out), npatch.long())
        c1 = _compare({"merge": lambda: quadtree_merge_raw(x, *args), "merge_with_map": lambda: quadtree_merge_raw(x, *args, want_map=True)},
                      a.window, a.rounds)
        dest = torch.empty((T, H, W, C), dtype=dtype, device=dev)
        c2 = _compare({"unmerge_tokens": lambda: sttm_amd.unmerge_tokens(feat, t2o, out=dest)}, a.window, a.rounds)
        assert torch.equal(dest.view(T * H * W, C), feat[t2o.flatten().long()])
        nbytes = (T * H * W + n_out) * C * eb
        for leg in c2.values():
            leg["bytes_per_s"] = round(nbytes / (leg["us"] * 1e-6), 1)
            leg["share_of_peak"] = round(leg["bytes_per_s"] / PEAK_BYTES_PER_S, 4)
        results.append(dict(
            dtype=str(dtype).replace("torch.", ""), C=C, T=T, H=H, W=W, n_out=n_out, algorithmic_bytes=nbytes,
            map_cost=dict(legs=c1, difference_us=round(c1["merge_with_map"]["us"] - c1["merge"]["us"], 3)),
            unmerge=dict(legs=c2)))
        print(json.dumps(results[-1]), flush=True)
    doc = dict(tool="tools/token_map_bench.py", device=torch.cuda.get_device_name(0), build_tag=_lib.build_tag(), torch=torch.__version__,
               window_s=a.window, rounds=a.rounds, peak_bytes_per_s=PEAK_BYTES_PER_S, results=results)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
