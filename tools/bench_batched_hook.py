"""The merge step of the batched quadtree hook (merge of the B videos + the ragged pack) against a Python loop of B batch-1 hook calls
followed by left padding, and the pack kernel (sttm_pack_merged_batch) alone, on the GPU.

    python tools/bench_batched_hook.py [--out FILE.json] [--reps N] [--B 8] [--C 3584]

Setting: B left-padded LLaVA-Video prompts, bf16, 14 x 14 grids, T drawn from 64..128 per row, system / instruction spans of different
lengths.  Times are HIP-event medians around whole host calls (the batched path includes its one wait for the token counts, the loop
its B waits).  Pack bytes = every valid row read once (system, merged, instruction) + the whole [B, L'max, C] block written, plus the
mask / positions / idx words; reported against the 8 TB/s HBM roofline."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

ROOF = 8e12


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
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--C", type=int, default=3584)
    args = ap.parse_args()
    from sttm_amd import _lib, patch_hooks
    from sttm_amd.quadtree_interface import (get_quadtree_features, get_quadtree_features_batch_reused, get_quadtree_features_into,
                                             pack_merged_batch)
    from sttm_amd.synth import synth_video
    dev, dt, B, C, H = torch.device("cuda:0"), torch.bfloat16, args.B, args.C, 14
    g = torch.Generator().manual_seed(0)
    Ts = [int(v) for v in torch.randint(64, 129, (B,), generator=g)]
    sys_n = [int(v) for v in torch.randint(0, 20, (B,), generator=g)]
    inst_n = [int(v) for v in torch.randint(5, 60, (B,), generator=g)]
    lens = [s + T * H * H + i for s, T, i in zip(sys_n, Ts, inst_n)]
    L = max(lens)
    pads = [L - n for n in lens]
    hs = torch.randn(B, L, C, generator=g).to(dev, dt)
    for b in range(B):
        vid = synth_video(Ts[b], C, H, H, seed=b, dtype=dt, device=dev)
        hs[b, pads[b] + sys_n[b]:pads[b] + sys_n[b] + Ts[b] * H * H] = vid.permute(0, 2, 3, 1).reshape(-1, C)
    mask = torch.zeros(B, L, dtype=torch.long, device=dev)
    for b in range(B):
        mask[b, pads[b]:] = 1
    pos = (mask.cumsum(-1) - 1).masked_fill(mask == 0, 1)
    vlen = [T * H * H for T in Ts]
    thr = (0.85, 0.55, 1, False)

    def batched():
        return patch_hooks.quadtree_merge_llava_batched(hs, pos, pads, sys_n, vlen, Ts, get_quadtree_features_batch_reused,
                                                        pack_merged_batch, *thr)

    def loop():
        outs = []
        for b in range(B):
            row = hs[b:b + 1, pads[b]:]
            outs.append(patch_hooks.quadtree_merge_llava(row, pos[b:b + 1, pads[b]:], sys_n[b], vlen[b], Ts[b], get_quadtree_features,
                                                         *thr, merge_into_fn=get_quadtree_features_into))
        Lout = max(o[0].shape[1] for o in outs)
        packed = hs.new_zeros((B, Lout, C))
        m2 = torch.zeros(B, Lout, dtype=torch.long, device=dev)
        p2 = torch.ones(B, Lout, dtype=torch.long, device=dev)
        for b, (o, q, _) in enumerate(outs):
            packed[b, Lout - o.shape[1]:] = o[0]
            m2[b, Lout - o.shape[1]:] = 1
            p2[b, Lout - o.shape[1]:] = q[0]
        return packed, m2, p2, [o[2] for o in outs]

    a, b_ = batched(), loop()
    exact = (torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1]) and torch.equal(a[2], b_[2])
             and all(torch.equal(x, y) for x, y in zip(a[3], b_[3])))
    t_batched = _event_us(batched, args.reps)
    t_loop = _event_us(loop, args.reps)
    # the merge alone and the pack alone
    videos = [patch_hooks._video_view(hs[b, pads[b] + sys_n[b]:pads[b] + sys_n[b] + vlen[b]], Ts[b], H, H) for b in range(B)]
    t_merge = _event_us(lambda: get_quadtree_features_batch_reused(videos, *thr), args.reps)
    res = get_quadtree_features_batch_reused(videos, *thr)
    geom = [(pads[b], sys_n[b], vlen[b], int(res[b][0].shape[0]), Ts[b], H, H) for b in range(B)]
    Lout = max(L - p - n + m for p, _, n, m, _, _, _ in geom)
    merged = [(f, t) for f, _, t in res]
    t_pack = _event_us(lambda: pack_merged_batch(hs, merged, geom, Lout, pos, _lib.PACK_POS_TRUNCATE), args.reps)
    eb = hs.element_size()
    valid = sum(L - p - n + m for p, _, n, m, _, _, _ in geom)
    nbytes = valid * C * eb + B * Lout * C * eb + B * Lout * 16 + valid * 8 + sum(g[3] for g in geom) * 16
    result = dict(B=B, C=C, dtype="bf16", T=Ts, grid=[H, H], L=L, Lout=Lout, merged_rows=[g[3] for g in geom],
                  bit_identical=exact, batched_merge_step_us=round(t_batched, 1), loop_merge_step_us=round(t_loop, 1),
                  speedup=round(t_loop / t_batched, 3), batch_merge_only_us=round(t_merge, 1), pack_us=round(t_pack, 1),
                  pack_bytes=nbytes, pack_TBps=round(nbytes / t_pack / 1e6, 3), pack_roofline_frac=round(nbytes / (t_pack * 1e-6) / ROOF, 3),
                  build_tag=_lib.build_tag())
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
