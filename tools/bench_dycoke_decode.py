"""DyCoke stage 2: the attention part of one decode step on the GPU, three ways, at Qwen2-7B attention shapes.

    python tools/bench_dycoke_decode.py [--out profiles/dycoke_decode_bench.json] [--reps 30] [--no-allowances]

Setting: 28 layers, Hq = 28, Hkv = 4, D = 128, bf16, start = 14, n0 = 25 088 visual tokens before stage 1, 11 978 after it
(sttm_dycoke_out_rows(128, 196, 58)), 60 instruction tokens, dycoke_l = 3, dycoke_p = 0.8: Lk = 12 053 keys, 5 017 + 14 kept.

  kernels      decode_attn_scores (layer l - 1) + select_keep + 25 x gathered_decode_attention
  as written   what dycoke_attn_monkey_patch.py does per step: layer l - 1 in eager mode (full attention matrix and its output),
               mean over heads, window, topk, .tolist(); per layer >= l torch.tensor(list), two gathers of the cache, sdpa
  no pruning   scaled_dot_product_attention over the full cache for the 25 layers (what not pruning costs)

Times are HIP-event medians over whole steps issued from the host (host work and its synchronisations included: they are part of the
step), after warm-up of every shape; the spread is the 10th / 90th percentile.  The parent commit cannot run the pattern, so the
as-written torch composition on the same device in the same process is the baseline.  The allowances of tests/test_hip_dycoke_decode.py
(reference against reference) and the kernels' measured errors are recorded alongside."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _steps_us(fn, reps, warm=5):
    for _ in range(warm):
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
    times.sort()
    return {"median_us": round(statistics.median(times), 1), "p10_us": round(times[len(times) // 10], 1),
            "p90_us": round(times[(9 * len(times)) // 10], 1), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "dycoke_decode_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-allowances", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from sttm_amd import _lib
    from sttm_amd.dycoke_decode import decode_attn_scores, gathered_decode_attention, num_keep_of, select_keep
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    layers, Hq, Hkv, D, start, n0, l, p, inst = 28, 28, 4, 128, 14, 25088, 3, 0.8, 60
    merged = int(_lib.load().sttm_dycoke_out_rows(128, 196, 58))
    Lk = start + merged + inst + 1
    G, scale, num_keep, late = Hq // Hkv, D ** -0.5, num_keep_of(n0, p), layers - l
    g = torch.Generator(device=dev).manual_seed(0)
    q = [torch.randn(1, Hq, 1, D, generator=g, device=dev).to(dt) for _ in range(late + 1)]
    K = [torch.randn(1, Hkv, Lk, D, generator=g, device=dev).to(dt) for _ in range(late + 1)]
    V = [torch.randn(1, Hkv, Lk, D, generator=g, device=dev).to(dt) for _ in range(late + 1)]
    sdpa = torch.nn.functional.scaled_dot_product_attention

    def kernels_step():
        keep = select_keep(decode_attn_scores(q[0], K[0], scale), start, n0, num_keep)
        return [gathered_decode_attention(q[i], K[i], V[i], keep, scale) for i in range(1, late + 1)]

    def as_written_step():
        kk, vv = K[0].repeat_interleave(G, dim=1), V[0].repeat_interleave(G, dim=1)           # eager layer l - 1 (:410-411)
        w = torch.softmax(torch.matmul(q[0], kk.transpose(2, 3)) * scale, dim=-1, dtype=torch.float32).to(dt)
        torch.matmul(w, vv)
        att = w.mean(1)[0, -1][start:start + n0]                                              # :80-83
        top = torch.topk(att, num_keep, sorted=False)[1] + start                              # :69
        rng = torch.arange(Lk, device=dev)
        keep = torch.cat([rng[:start], top, rng[start + n0:]]).tolist()                       # :72-77
        outs = []
        for i in range(1, late + 1):                                                          # :54-60, every layer >= l
            ik = torch.tensor(keep, device=dev).view(1, 1, -1, 1).expand(1, Hkv, -1, D)
            iv = torch.tensor(keep, device=dev).view(1, 1, -1, 1).expand(1, Hkv, -1, D)
            outs.append(sdpa(q[i], torch.gather(K[i], 2, ik), torch.gather(V[i], 2, iv), scale=scale, enable_gqa=True))
        return outs

    def plain_step():
        return [sdpa(q[i], K[i], V[i], scale=scale, enable_gqa=True) for i in range(1, late + 1)]

    # faster and different is not faster: the kernels' step against the as-written one on the same inputs
    a, b = kernels_step(), as_written_step()
    diff = max(float((x.transpose(1, 2).float() - y.float()).abs().max()) for x, y in zip(a, b))
    res = {"setting": {"layers": layers, "Hq": Hq, "Hkv": Hkv, "D": D, "dtype": "bf16", "start": start, "n0": n0, "merged_visual": merged,
                       "instruction": inst, "Lk": Lk, "dycoke_l": l, "dycoke_p": p, "num_keep": num_keep, "n_keep": start + num_keep,
                       "gathered_layers": late},
           "max_abs_diff_kernels_vs_as_written": diff}
    # alternate the three legs twice, keep both rounds
    for rnd in (1, 2):
        res[f"kernels_step_round{rnd}"] = _steps_us(kernels_step, args.reps)
        res[f"as_written_torch_step_round{rnd}"] = _steps_us(as_written_step, args.reps)
        res[f"plain_full_cache_sdpa_round{rnd}"] = _steps_us(plain_step, args.reps)
    keep = select_keep(decode_attn_scores(q[0], K[0], scale), start, n0, num_keep)
    score = decode_attn_scores(q[0], K[0], scale)
    res["scores_call"] = _steps_us(lambda: decode_attn_scores(q[0], K[0], scale), args.reps)
    res["select_call"] = _steps_us(lambda: select_keep(score, start, n0, num_keep), args.reps)
    res["gathered_call"] = _steps_us(lambda: gathered_decode_attention(q[1], K[1], V[1], keep, scale), args.reps)
    res["speedup_over_as_written"] = round(res["as_written_torch_step_round2"]["median_us"] / res["kernels_step_round2"]["median_us"], 2)
    res["kernels_over_plain_sdpa"] = round(res["kernels_step_round2"]["median_us"] / res["plain_full_cache_sdpa_round2"]["median_us"], 2)
    res["score_logits"] = "workspace of Hq * Lk floats between the two passes (the recomputing variant was not built, so not measured)"
    try:
        res["clock_mhz_after_run"] = torch.cuda.clock_rate()
    except Exception as e:       # noqa: BLE001
        res["clock_mhz_after_run"] = f"not read ({type(e).__name__})"
    if not args.no_allowances:
        from tests import test_hip_dycoke_decode as T
        from tests import _dycoke_decode_ref as R
        base, eps = T.score_allowance()
        worst = 0.0
        for n, (cdt, hq, hkv, d, lk, strided) in enumerate(T.SCORE_CASES):
            qq, kk, _ = T.make_qkv(cdt, hq, hkv, d, lk, strided, n)
            worst = max(worst, T._rel(decode_attn_scores(qq, kk, d ** -0.5), R.decode_attn_scores_ref(qq.double(), kk.double(), d ** -0.5)))
        res["scores_rel_dev_float32_restatement_vs_float64"] = base
        res["scores_allowance"] = eps
        res["scores_rel_dev_kernel_vs_float64"] = worst
        for cdt in T.DTYPES:
            base, tol = T.attn_allowance(cdt)
            worst = 0.0
            for n, (c2, hq, hkv, d, lk, strided) in enumerate(T.ATTN_CASES):
                if c2 != cdt:
                    continue
                qq, kk, vv = T.make_qkv(c2, hq, hkv, d, lk, strided, 900 + n)
                for kp in T._keep_lists(lk, n).values():
                    ref = R.gathered_decode_attention_ref(qq.double(), kk.double(), vv.double(), kp, d ** -0.5)
                    worst = max(worst, T._attn_err(gathered_decode_attention(qq, kk, vv, kp, d ** -0.5), ref))
            name = str(cdt).replace("torch.", "")
            res[f"gathered_err_torch_sdpa_vs_float64_{name}"] = base
            res[f"gathered_allowance_{name}"] = tol
            res[f"gathered_err_kernel_vs_float64_{name}"] = worst
    res["build_tag"] = _lib.build_tag()
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
