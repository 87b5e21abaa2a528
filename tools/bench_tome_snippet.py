"""Per-frame / per-snippet ToMe against the only route the per-clip API offers to the same result, on the GPU.

    python tools/bench_tome_snippet.py [--out profiles/tome_snippet_bench.json] [--window 0.5] [--rounds 3]

At T = 128, 14 x 14, fp32 C = 1024 and bf16 C = 3584, S in {1, 4, 16}, p in {0.5, 0.7}:
  (a) snippet    get_tome_features_snippet(x, p, S): all snippets in one set of launches per merge iteration (S = 16 is above the
                 segment kernels' cap: the per-clip step per snippet into shared output blocks, dealt out to two side streams)
  (b) host loop  get_tome_features(x[g*S:(g+1)*S], p, "video") for every snippet, ids offset, results concatenated
  (c) video      get_tome_features(x, p, "video") on the whole clip, for scale (a different result: one snippet of 128 frames)
One process; after warm-up the three are timed in turn, round after round, each over a window of at least --window seconds of
back-to-back calls between two device events (host work included: it is part of the call).  (b) is timed twice per round: the
relative difference of its two medians is the run-to-run spread.  (a) and (b) must agree under the rule of
tests/test_hip_tome_snippet.py (fp32: at most one near-tie per snippet; bf16: `_assert_tome16`'s shares).
Required: at S = 1 and S = 4 (a) takes at most half the time of (b); at S = 16 (a) is not slower than (b) beyond the spread.
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _window_ms(fn, seconds, calls):
    """Milliseconds per call over a window of `calls` back-to-back calls (at least `seconds` long once calibrated)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def _calibrate(fn, seconds):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    one = _window_ms(fn, seconds, 3)
    return max(3, math.ceil(seconds * 1e3 / one))


def _agreement(fa, ia, fb, ib, lens, lowp):
    """Per snippet: kept ids that differ and common ids whose rows differ (fp32: 1e-5 absolute; 16-bit: 2 ulp of the dtype)."""
    fa, ia, fb, ib = fa.cpu().float(), ia.cpu(), fb.cpu().float(), ib.cpu()
    tol = None if not lowp else (2.0 ** -6 if lowp == "bfloat16" else 2.0 ** -9)
    ids_diff, rows_diff, worst_ids, worst_rows, o = 0, 0, 0, 0, 0
    for n in lens:
        sa, sb = ia[o:o + n], ib[o:o + n]
        oa, ob = torch.argsort(sa), torch.argsort(sb)
        common = sorted(set(sa.tolist()) & set(sb.tolist()))
        sel = torch.tensor(common, dtype=torch.int64)
        ra, rb = fa[o:o + n][oa][torch.searchsorted(sa[oa], sel)], fb[o:o + n][ob][torch.searchsorted(sb[ob], sel)]
        if lowp:
            bad = int(((ra - rb).abs() / rb.abs().clamp_min(1.0) > tol).any(dim=1).sum())
        else:
            bad = int(((ra - rb).abs().amax(dim=1) > 1e-5).sum())
        ids_diff += n - len(common)
        rows_diff += bad
        worst_ids, worst_rows = max(worst_ids, n - len(common)), max(worst_rows, bad)
        o += n
    return dict(kept=int(sum(lens)), ids_differ=ids_diff, rows_differ=rows_diff, worst_snippet_ids=worst_ids, worst_snippet_rows=worst_rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "tome_snippet_bench.json"))
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="", help="dtype:S:p of one shape (for a profiler run), e.g. float32:1:0.7")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from sttm_amd import _lib, get_tome_features, get_tome_features_snippet
    from sttm_amd.synth import synth_video
    dev = torch.device("cuda:0")
    T, H, W = 128, 14, 14
    hw = H * W
    results, failures = [], []
    for dtype, C in ((torch.float32, 1024), (torch.bfloat16, 3584)):
        name = str(dtype).replace("torch.", "")
        x = synth_video(T, C, H, W, seed=178, dtype=dtype).to(dev)
        for S in (1, 4, 16):
            for p in (0.5, 0.7):
                if args.only and args.only != f"{name}:{S}:{p}":
                    continue
                ranges = [(t0, min(t0 + S, T)) for t0 in range(0, T, S)]
                lens = [math.ceil((t1 - t0) * hw * (1 - p)) for t0, t1 in ranges]

                def snippet():
                    return get_tome_features_snippet(x, p, S)

                def host_loop():
                    parts = [get_tome_features(x[t0:t1], p, "video") for t0, t1 in ranges]
                    return torch.cat([q[0] for q in parts]), torch.cat([q[1] + t0 * hw for q, (t0, _t1) in zip(parts, ranges)])

                def video():
                    return get_tome_features(x, p, "video")

                agree = _agreement(*snippet(), *host_loop(), lens, None if dtype == torch.float32 else name)
                if dtype == torch.float32:
                    ok = agree["worst_snippet_ids"] <= 1 and agree["worst_snippet_rows"] <= 2
                else:
                    n = agree["kept"]
                    ok = agree["ids_differ"] <= max(1, -(-n * 2 // 1000)) and agree["rows_differ"] <= max(2, -(-n * 5 // 1000))
                calls = {k: _calibrate(f, args.window) for k, f in (("a", snippet), ("b", host_loop), ("c", video))}
                ms = {"a": [], "b": [], "b2": [], "c": []}
                for _ in range(args.rounds):
                    ms["a"].append(_window_ms(snippet, args.window, calls["a"]))
                    ms["b"].append(_window_ms(host_loop, args.window, calls["b"]))
                    ms["c"].append(_window_ms(video, args.window, calls["c"]))
                    ms["b2"].append(_window_ms(host_loop, args.window, calls["b"]))
                med = {k: statistics.median(v) for k, v in ms.items()}
                spread = abs(med["b"] - med["b2"]) / min(med["b"], med["b2"])
                b_ms = min(med["b"], med["b2"])
                row = dict(dtype=name, C=C, T=T, H=H, W=W, S=S, p=p, snippet_ms=round(med["a"], 4), host_loop_ms=round(b_ms, 4),
                           host_loop_repeat_ms=round(max(med["b"], med["b2"]), 4), video_ms=round(med["c"], 4),
                           host_loop_over_snippet=round(b_ms / med["a"], 2), spread=round(spread, 4),
                           calls_per_window=calls, windows_ms={k: [round(v, 4) for v in vs] for k, vs in ms.items()},
                           segment_kernels=S * hw <= _lib.TOME_SEGMENT_MAX_TOKENS, agreement=agree, agreement_ok=ok)
                if S in (1, 4):
                    row["required"] = "snippet <= host loop / 2"
                    row["met"] = med["a"] <= b_ms / 2
                else:
                    row["required"] = "snippet <= host loop * (1 + spread)"
                    row["met"] = med["a"] <= b_ms * (1 + spread)
                if not (row["met"] and ok):
                    failures.append(f"{name} S={S} p={p}")
                results.append(row)
                print(json.dumps({k: row[k] for k in ("dtype", "S", "p", "snippet_ms", "host_loop_ms", "video_ms", "host_loop_over_snippet",
                                                      "spread", "met", "agreement_ok")}), flush=True)
    doc = dict(tool="tools/bench_tome_snippet.py", device=torch.cuda.get_device_name(0), build_tag=_lib.build_tag(), torch=torch.__version__,
               segment_cap_tokens=_lib.TOME_SEGMENT_MAX_TOKENS, window_s=args.window, rounds=args.rounds, results=results, failures=failures)
    if not args.only:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
    if failures:
        raise SystemExit("requirement missed at: " + ", ".join(failures))


if __name__ == "__main__":
    main()
