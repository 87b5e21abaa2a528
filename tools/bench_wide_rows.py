"""Token rows wider than one workgroup (the channel-tiled spatial stage, csrc/spatial_wide.inc) against the widest one-workgroup rows,
on the GPU: HIP-event time of whole calls, one call per video (get_quadtree_features) and through get_quadtree_features_batch.

    python tools/bench_wide_rows.py [--out FILE.json] [--reps N] [--wide-lanes 0|256|512|1024] [--quick]

Each line: us per video (median over reps, events around the whole call), the algorithmic bytes of one video
B = eb*C*T*H*W (read once) + eb*C*N' + 24*N' (features, num_patches, tlbr written once), and B / time as a fraction of the
8 TB/s HBM roofline.  The pairs "fp32 C = 8192 / fp32 C = 4096" and "bf16 C = 16384 / bf16 C = 8192" are reported as factors."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

ROOF = 8e12

SHAPES = [
    # (name, T, C, H, W, dtype, threshold, temporal)
    ("f32_C4096_T128", 128, 4096, 14, 14, torch.float32, 0.85, 0.55),
    ("f32_C8192_T128", 128, 8192, 14, 14, torch.float32, 0.85, 0.55),
    ("f32_C4096_T180", 180, 4096, 14, 14, torch.float32, 0.94, 0.82),
    ("f32_C8192_T180", 180, 8192, 14, 14, torch.float32, 0.94, 0.82),
    ("bf16_C8192_T128", 128, 8192, 14, 14, torch.bfloat16, 0.85, 0.55),
    ("bf16_C16384_T128", 128, 16384, 14, 14, torch.bfloat16, 0.85, 0.55),
    ("f32_C8192_T128_20x36", 128, 8192, 20, 36, torch.float32, 0.85, 0.60),
]
PAIRS = [("f32_C8192_T128", "f32_C4096_T128"), ("f32_C8192_T180", "f32_C4096_T180"), ("bf16_C16384_T128", "bf16_C8192_T128")]


def _event_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=8, help="videos per get_quadtree_features_batch call")
    ap.add_argument("--wide-lanes", type=int, default=0, help="sttm_configure wide_lanes for the whole run (0 = automatic)")
    ap.add_argument("--quick", action="store_true", help="T = 128 14x14 fp32 pair only, no batch leg")
    args = ap.parse_args()
    from sttm_amd import _lib, get_quadtree_features
    from sttm_amd.quadtree_interface import get_quadtree_features_batch
    from sttm_amd.synth import synth_video
    dev = torch.device("cuda:0")
    _lib.configure(wide_lanes=args.wide_lanes)
    shapes = SHAPES[:2] if args.quick else SHAPES
    lines = []
    res = {}
    for name, T, C, H, W, dt, thr, tthr in shapes:
        nvid = 1 if args.quick else args.batch
        xs = [synth_video(T, C, H, W, seed=700 + i, dtype=dt).to(dev) for i in range(min(nvid, 3))]
        xs = [xs[i % len(xs)] for i in range(nvid)]
        n_out = get_quadtree_features(xs[0], thr, tthr, 1)[0].shape[0]
        eb = xs[0].element_size()
        B = eb * C * T * H * W + eb * C * n_out + 24 * n_out
        med, best = _event_us(lambda: get_quadtree_features(xs[0], thr, tthr, 1), args.reps)
        line = dict(shape=name, T=T, C=C, H=H, W=W, dtype=str(dt).split(".")[-1], wide_lanes=args.wide_lanes, n_out=n_out,
                    algorithmic_MB=round(B / 1e6, 2), one_call_us=round(med, 1), one_call_min_us=round(best, 1),
                    one_call_roofline=round(B / (med * 1e-6) / ROOF, 3))
        if not args.quick:
            bmed, bbest = _event_us(lambda: get_quadtree_features_batch(xs, thr, tthr, 1), max(3, args.reps // 3))
            line.update(batch_videos=nvid, batch_us_per_video=round(bmed / nvid, 1),
                        batch_roofline=round(B * nvid / (bmed * 1e-6) / ROOF, 3))
        print(json.dumps(line), flush=True)
        lines.append(line)
        res[name] = line
        del xs
        torch.cuda.empty_cache()
    factors = []
    for wide, narrow in PAIRS:
        if wide in res and narrow in res:
            f = dict(wide=wide, narrow=narrow, one_call_factor=round(res[wide]["one_call_us"] / res[narrow]["one_call_us"], 2))
            if "batch_us_per_video" in res[wide]:
                f["batch_factor"] = round(res[wide]["batch_us_per_video"] / res[narrow]["batch_us_per_video"], 2)
            print(json.dumps(f), flush=True)
            factors.append(f)
    _lib.configure(wide_lanes=0)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(dict(build_tag=_lib.load().sttm_build_tag().decode(), device=torch.cuda.get_device_name(0), lines=lines,
                           factors=factors), fh, indent=1)


if __name__ == "__main__":
    main()
