#!/usr/bin/env python3
"""Benchmark of the STTM merge hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--mode batch|dropin] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json metric): synth-v1 videos of 128 frames x 14x14 tokens x 1024 channels, fp32, in the
production layout (channels-last view), full STTM = quadtree spatial merge (thr 0.85, root_level 1) +
temporal merge (thr 0.55) -- the LLaVA-Video-7B / Video-MME "50 % budget" preset of the reference
(scripts/eval/run_vidqa.sh:58).  A step = `--videos-per-step` videos, inputs resident in HBM, every video's outputs
(incl. its host-visible token count) produced.  `--mode batch` (default): get_quadtree_features_batch, `--batch`
independent videos per call, which the library deals out to its internal streams (stage-skewed; identical outputs);
`--mode dropin`: get_quadtree_features, one video per call on one stream (the definition of `value` in rounds 1-4).
A plain run sets up, warms up, times the K steps and prints the headline line; `--full` adds every other leg (the mode the
timed region does not run, the threaded / ToMe / hook extensions, the configurations, the per-kernel roofline leg and the
CPU baseline with its parity check), each of which `--no-*` can skip again.  Videos are independent, so N GPUs each take
their own videos (weak scaling); the only collective is the final gather of the per-video token counts over RCCL
(with --validate also the padded merged-token indices).

`python bench.py --gpus N` without a torchrun environment spawns the N ranks itself.
Prints ONE JSON line on rank 0 (see DESIGN.md section "Measurement" for every field).
"""
import argparse
import json
import os
import socket
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8 TB/s (spec)
HBM_COPY_GBS = 6300.0        # MI355X_MICROARCH.md: what a plain device copy achieves on this part (~6.3 TB/s)
L3_BYTES = 256e6             # Infinity Cache: pools of the timed legs are sized past it
MFMA_F32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: fp32-input MFMA = the fp32 vector rate
MFMA_F16_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: BF16/FP16 MFMA, dense (32x32x16)
KERNELS = ["quadtree_spatial", "temporal_pairs_labels", "labels_standalone", "group_mean"]
# fp16 product terms per fp32 ToMe score (the library's tome_split switch: 2 -> three terms, the default; 1 -> four)
TOME_TERMS = {"1": 4, "2": 3, "3": 4, "4": 4, "5": 3, "6": 3, "7": 3}.get(os.environ.get("STTM_TOME_SPLIT", "2"), 4)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--videos-per-step", type=int, default=1536,
                    help="videos per step: 20 steps of 1536 videos keep the timed region above 2 s")
    ap.add_argument("--pool", type=int, default=8, help="distinct videos resident per GPU (> L3 capacity in total)")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="budget of the CPU-baseline sample")
    ap.add_argument("--profile-calls", type=int, default=1024, help="calls of the per-kernel (HIP event) leg")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extensions", "--no-batched", dest="no_extensions", action="store_true",
                    help="skip the batched / threaded / ToMe legs (e.g. under rocprofv3)")
    ap.add_argument("--no-configs", action="store_true", help="skip the per-configuration leg (BASELINE configs 1/2/4/5 + production shapes)")
    ap.add_argument("--mode", choices=("batch", "dropin"), default="batch",
                    help="what the timed region (`value`) runs: 'batch' = get_quadtree_features_batch, --batch videos per call, dealt out to "
                         "the library's internal streams (stage-skewed; identical outputs); 'dropin' = get_quadtree_features, one video per "
                         "call on one stream (rounds 1-4's headline).  With --full the other mode is reported next to it.")
    ap.add_argument("--batch", type=int, default=96, help="videos per get_quadtree_features_batch call in 'batch' mode")
    ap.add_argument("--validate", action="store_true",
                    help="after the timed region, all-gather the padded merged-token indices of a sample of videos over the ranks "
                         "and check them against each rank's own recomputation")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run the other mode, the extension legs, the configurations, the per-kernel roofline "
                         "leg and the CPU baseline (each can be skipped with its --no-* switch)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path returned in its last step to DIR/<name>.npy (float32 / float64, rank 0)")
    return ap.parse_args()


_T0 = time.perf_counter()


def log(msg):
    if int(os.environ.get("RANK", "0")) == 0:
        print(f"[bench +{time.perf_counter() - _T0:7.2f}s] {msg}", file=sys.stderr, flush=True)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _pci_address(props):
    return "%04x:%02x:%02x.0" % (getattr(props, "pci_domain_id", 0), props.pci_bus_id, getattr(props, "pci_device_id", 0))


def pin_to_gpu_numa_node(local_rank, local_world=None, sysfs_root="/sys"):
    """Pin this rank's host threads to its share of the CPUs of its GPU's NUMA node (the launch thread spins on a pinned-memory
    flag after every video: it should sit next to the GPU's PCIe root, and ranks whose GPUs share a node get DISJOINT shares of
    it -- sttm_amd.distributed.numa_cpu_sets, unit-tested against a fake sysfs tree).  Best effort -- returns a description, or
    None when the topology is not exposed (containers often hide it)."""
    try:
        import torch
        from sttm_amd.distributed import numa_cpu_sets, read_gpu_numa_topology
        n_local = local_world or int(os.environ.get("LOCAL_WORLD_SIZE", "0")) or max(local_rank + 1, 1)
        n_local = min(max(n_local, local_rank + 1), torch.cuda.device_count())
        addrs = [_pci_address(torch.cuda.get_device_properties(i)) for i in range(n_local)]
        nodes, node_cpus = read_gpu_numa_topology(addrs, sysfs_root)
        mine = numa_cpu_sets(nodes, node_cpus, set(os.sched_getaffinity(0)))[local_rank]
        if not mine:
            return None
        os.sched_setaffinity(0, mine)
        return {"numa_node": nodes[local_rank], "cpus": len(mine), "ranks_on_this_node": sum(1 for n in nodes if n == nodes[local_rank])}
    except Exception:  # noqa: BLE001
        return None


def host_cpu_facts():
    """logical CPUs visible to this process and physical cores of the host (distinct (physical id, core id) pairs)."""
    logical = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    cores, model = set(), None
    try:
        phys = core = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name") and model is None:
                model = line.split(":", 1)[1].strip()
            elif line.startswith("physical id"):
                phys = line.split(":", 1)[1].strip()
            elif line.startswith("core id"):
                core = line.split(":", 1)[1].strip()
            elif not line.strip():
                if phys is not None and core is not None:
                    cores.add((phys, core))
                phys = core = None
    except OSError:
        pass
    return {"logical_cpus": logical, "physical_cores": len(cores) or None, "model": model}


# BASELINE.json configurations next to the headline (C3): name, T, C, H, W, dtype, spatial thr, temporal thr -- the presets of
# the reference's scripts/eval/run_vidqa.sh:44,56,58,84,89 -- and the hidden-state shapes the hooks really hand over
# (token_merging_monkey_patch/quadtree_attn_monkey_patch.py:98: bf16, C = 3584 for the 7B and 8192 for the 72B model).
CONFIGS = [
    ("C1 T=8 14x14x1024 f32 spatial 0.85", 8, 1024, 14, 14, "float32", 0.85, -1.0),
    ("C2 T=64 14x14x1024 f32 STTM(0.85,0.65)", 64, 1024, 14, 14, "float32", 0.85, 0.65),
    ("C4 T=128 20x36x1024 f32 STTM(0.85,0.60)", 128, 1024, 20, 36, "float32", 0.85, 0.60),
    ("C4 T=128 18x26x1024 f32 STTM(0.85,0.60)", 128, 1024, 18, 26, "float32", 0.85, 0.60),
    ("C4 T=128 13x24x1024 f32 STTM(0.85,0.60)", 128, 1024, 13, 24, "float32", 0.85, 0.60),
    ("C5 T=180 14x14x1024 f32 STTM(0.94,0.82)", 180, 1024, 14, 14, "float32", 0.94, 0.82),
    ("prod T=128 14x14x3584 bf16 STTM(0.85,0.55)", 128, 3584, 14, 14, "bfloat16", 0.85, 0.55),
    ("prod T=128 14x14x8192 bf16 STTM(0.85,0.55)", 128, 8192, 14, 14, "bfloat16", 0.85, 0.55),
    # not a BASELINE configuration: 6-level trees (a 9th entry = root_level; 36 x 64 tokens at root_level 0: root cells of up to 32 x 32
    # leaves), the shape the round-3 review measures the several-workgroups-per-root-cell spatial stage on
    ("deep T=16 36x64x1024 f32 STTM(0.85,0.55) root_level 0 (6-level trees)", 16, 1024, 36, 64, "float32", 0.85, 0.55, 0),
]


def run_configs(dev, rank, world, timed, log):
    """videos/s, algorithmic bytes B (read every token once, write every merged token once + 24 B of metadata) and
    B / time / 8 TB/s for every secondary configuration, through the drop-in API with device-resident inputs.  The pool of every
    shape holds >= 300 MB of distinct videos (> the 256 MB Infinity Cache: a video is not cache-resident from its previous use;
    round 3 used 3 videos per shape, which left C1 and C2 inside the cache).  The ToMe half of config 5 (T=180, r=0.5) rides along
    with its flop roofline."""
    from sttm_amd.quadtree_interface import get_quadtree_features, get_quadtree_features_batch
    from sttm_amd.synth import synth_video
    from sttm_amd.tome_interface import get_tome_features
    out = []
    for cfg in CONFIGS:
        name, T, C, H, W, dtn, thr, tthr = cfg[:8]
        root = cfg[8] if len(cfg) > 8 else 1
        dt = getattr(torch, dtn)
        eb = 4 if dt == torch.float32 else 2
        npool = max(3, int(-(-300e6 // (eb * C * T * H * W))))
        pool = [synth_video(T, C, H, W, seed=7000 + 100 * rank + i, dtype=dt, device=dev, gen_device=dev) for i in range(npool)]
        kept = [get_quadtree_features(x, thr, tthr, root)[0].shape[0] for x in pool]       # warm-up + N' of each
        reps = max(24, 2 * npool, min(300, int(0.25 / (5e-8 * T * H * W * C / 1024 + 2e-5))))

        def run(pool=pool, reps=reps, thr=thr, tthr=tthr, npool=npool, root=root):
            for i in range(reps):
                get_quadtree_features(pool[i % npool], thr, tthr, root)
        vps = timed(run, reps) / world                                                      # per GPU
        # the same videos through the batch entry point (48 per call, cycling the pool)
        nb = 48 if eb * C * T * H * W < 400e6 else 16
        blist = [pool[i % npool] for i in range(nb)]
        get_quadtree_features_batch(blist, thr, tthr, root)          # warm-up with the FULL list: the call's three output blocks and its scratch
                                                                       # (tens of GB for the large grids) come out of the caching allocator afterwards
        breps = max(1, reps // nb + 1)

        def run_b(blist=blist, breps=breps, thr=thr, tthr=tthr, root=root):
            for _ in range(breps):
                get_quadtree_features_batch(blist, thr, tthr, root)
        bvps = timed(run_b, breps * nb) / world
        n_out = sum(kept) / len(kept)
        B = eb * C * T * H * W + eb * C * n_out + 24 * n_out
        out.append({"config": name, "videos_per_s_per_gpu": round(vps, 1), "us_per_video": round(1e6 / vps, 1),
                    "batch_videos_per_s_per_gpu": round(bvps, 1), "batch_frac": round(B * bvps / 1e9 / HBM_PEAK_GBS, 4),
                    "keep_ratio": round(n_out / (T * H * W), 4), "algorithmic_MB": round(B / 1e6, 2), "pool_videos": npool,
                    "pool_MB": round(npool * eb * C * T * H * W / 1e6, 1),
                    "achieved_GBs": round(B * vps / 1e9, 1), "frac": round(B * vps / 1e9 / HBM_PEAK_GBS, 4),
                    "frac_of_copy_rate": round(B * vps / 1e9 / HBM_COPY_GBS, 4)})
        log(f"config {name}: {vps:.1f} videos/s one call per video (frac {out[-1]['frac']}), {bvps:.1f} batch (frac {out[-1]['batch_frac']})")
        del pool, blist
    # the step before the path: the merge starting from the UNPOOLED projector tokens [T, 729, C] bf16 (27 x 27 per frame,
    # llava/eval/video_feat_llavavideo.py:89-95 behind the projector): get_2dPool fused into the spatial kernel's leaf load against the
    # two-step form (sttm_pool2d writes the 14 x 14 map, the merge reads it back).  B = read every SOURCE token once + write every merged token.
    from sttm_amd import get_quadtree_features_from_pooled_input
    from sttm_amd.upstream import get_2dPool
    T, C, side = 128, 3584, 27
    npool = 3
    g = torch.Generator(device=dev).manual_seed(4242 + rank)
    src = []
    for i in range(npool):
        v = synth_video(T, C, 14, 14, seed=7300 + i, dtype=torch.bfloat16, device=dev, gen_device=dev)      # [T, C, 14, 14] view of [T, 14, 14, C]
        up = torch.nn.functional.interpolate(v.float(), size=(side, side), mode="bilinear").to(torch.bfloat16)
        src.append((up + 0.02 * torch.randn(up.shape, device=dev, generator=g).to(torch.bfloat16)).permute(0, 2, 3, 1).reshape(T, side * side, C).contiguous())
        del v, up
    kept = [get_quadtree_features_from_pooled_input(x, 0.85, 0.55, 1)[0].shape[0] for x in src]
    reps = 24

    def run_fused():
        for i in range(reps):
            get_quadtree_features_from_pooled_input(src[i % npool], 0.85, 0.55, 1)

    def run_two_step():
        for i in range(reps):
            pooled = get_2dPool(src[i % npool], stride=2, mode="bilinear")
            get_quadtree_features(pooled.reshape(T, 14, 14, C).permute(0, 3, 1, 2), 0.85, 0.55, 1)
    run_two_step()
    vps_f, vps_2 = timed(run_fused, reps) / world, timed(run_two_step, reps) / world
    n_out = sum(kept) / len(kept)
    B = 2 * C * T * side * side + 2 * C * n_out + 24 * n_out
    out.append({"config": f"from [T,{side * side},C] bf16: T={T} {side}x{side}x{C} -> bilinear 14x14 -> STTM(0.85,0.55), pool fused into the leaf load",
                "videos_per_s_per_gpu": round(vps_f, 1), "us_per_video": round(1e6 / vps_f, 1),
                "two_step_us_per_video": round(1e6 / vps_2, 1), "keep_ratio": round(n_out / (T * 196), 4),
                "algorithmic_MB": round(B / 1e6, 2), "pool_videos": npool, "pool_MB": round(npool * 2 * C * T * side * side / 1e6, 1),
                "achieved_GBs": round(B * vps_f / 1e9, 1), "frac": round(B * vps_f / 1e9 / HBM_PEAK_GBS, 4),
                "frac_of_copy_rate": round(B * vps_f / 1e9 / HBM_COPY_GBS, 4)})
    log(f"config from [T,729,C] bf16: fused {1e6 / vps_f:.1f} us, two-step {1e6 / vps_2:.1f} us per video, frac {out[-1]['frac']}")
    del src
    # config 5's ToMe half: T = 180, ratio 0.5 (run_vidqa.sh:44), fp32 and the bf16 hidden states of production
    T, C, H, W = 180, 1024, 14, 14
    n_tok = T * H * W
    flops = 2.0 * ((n_tok + 1) // 2) * (n_tok // 2) * C
    for dtn, peak in (("float32", MFMA_F16_PEAK_TFLOPS / TOME_TERMS), ("bfloat16", MFMA_F16_PEAK_TFLOPS)):
        pool = [synth_video(T, C, H, W, seed=7100 + i, dtype=getattr(torch, dtn), device=dev, gen_device=dev) for i in range(2)]
        get_tome_features(pool[0], 0.5, "video")
        reps = 12

        def run_t(pool=pool, reps=reps):
            for i in range(reps):
                get_tome_features(pool[i % 2], 0.5, "video")
        vps = timed(run_t, reps) / world
        from sttm_amd.tome_interface import get_tome_features_batch
        get_tome_features_batch([pool[i % 2] for i in range(reps)], 0.5, "video")

        def run_tb(pool=pool, reps=reps):
            get_tome_features_batch([pool[i % 2] for i in range(reps)], 0.5, "video")
        bvps = timed(run_tb, reps) / world
        out.append({"config": f"C5 ToMe video r=0.5 T=180 14x14x1024 {dtn}", "videos_per_s_per_gpu": round(vps, 1),
                    "batch_videos_per_s_per_gpu": round(bvps, 1), "batch_frac": round(flops * bvps / 1e12 / peak, 4),
                    "us_per_video": round(1e6 / vps, 1), "bound": "mfma", "algorithmic_GFLOP": round(flops / 1e9, 1),
                    "achieved_TFLOPs": round(flops * vps / 1e12, 1), "peak_TFLOPs": peak, "frac": round(flops * vps / 1e12 / peak, 4)})
        log(f"config ToMe T=180 {dtn}: {vps:.1f} videos/s one call per video (frac {out[-1]['frac']}), {bvps:.1f} over two side streams (frac {out[-1]['batch_frac']})")
        del pool
    torch.cuda.empty_cache()
    return out


DUMP_ROWS = 1 << 20          # --dump-outputs: per-row outputs of at most this many merged tokens (40 B each with their index)
DUMP_FEATURE_ROWS = 4096     # ... and feature rows of at most this many (4 KiB each at C = 1024): < 64 MB in all


def dump_outputs(path, step_counts, last_call):
    """--dump-outputs: what the timed path returned to its caller in the last timed step, as .npy files.

    step_counts: the merged-token count N' of every video of the last step.  last_call: the (features [N', C], num_patches [N'],
    tlbr [N', 5]) triples of the step's LAST call -- the only results of the step still alive (the batch entry point writes every call
    into the same caller-owned blocks).  Their rows, concatenated video after video, are the dumped rows; past DUMP_ROWS /
    DUMP_FEATURE_ROWS of them a fixed seeded sample (sorted) stands for them, so equal outputs give equal files."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    n = [o[0].shape[0] for o in last_call]
    total = sum(n)
    off = [0]
    for k in n:
        off.append(off[-1] + k)

    def sample(cap, seed):
        if total <= cap:
            return torch.arange(total)
        return torch.randperm(total, generator=torch.Generator().manual_seed(seed))[:cap].sort().values

    def gather(i, idx):                                   # rows idx of the concatenation of output i over the videos
        parts = []
        for v, o in enumerate(last_call):
            sel = idx[(idx >= off[v]) & (idx < off[v + 1])] - off[v]
            if sel.numel():
                parts.append(o[i][sel.to(o[i].device)].cpu())
        return torch.cat(parts)

    rows, frows = sample(DUMP_ROWS, 1), sample(DUMP_FEATURE_ROWS, 2)
    row_sum = torch.cat([o[0].double().sum(1).cpu() for o in last_call])[rows]
    arrays = {"counts": torch.tensor(step_counts, dtype=torch.float64), "row_index": rows.double(),
              "num_patches": gather(1, rows).float(), "tlbr": gather(2, rows).float(), "feature_row_sum": row_sum,
              "feature_row_index": frows.double(), "features": gather(0, frows).float()}
    nbytes = 0
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a.numpy())
        nbytes += a.numel() * a.element_size()
    assert nbytes <= 64e6, f"--dump-outputs wrote {nbytes / 1e6:.1f} MB"
    return {"videos": len(step_counts), "videos_with_rows": len(n), "rows": total, "MB": round(nbytes / 1e6, 2)}


def main():
    args = parse()
    if args.gpus > 1 and "RANK" not in os.environ:
        if torch.cuda.is_available() and torch.cuda.device_count() < args.gpus:
            sys.exit(f"bench.py --gpus {args.gpus}: this node has {torch.cuda.device_count()} GPU(s)")
        # plain `python bench.py --gpus N`: start the launcher of N ranks (one process per GPU, RCCL over xGMI) as a child process --
        # this one has already initialised the HIP runtime above, so it must not be replaced in place
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
        import subprocess
        sys.exit(subprocess.run(cmd).returncode)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    assert world == args.gpus, f"--gpus {args.gpus} but the launcher started {world} ranks"
    assert torch.cuda.is_available(), "bench.py needs an MI355X (no CPU fallback)"
    if torch.cuda.device_count() < args.gpus:
        # fail fast and clearly (one process per GPU of ONE node: there is nothing to fall back to)
        sys.exit(f"bench.py --gpus {args.gpus}: this node shows {torch.cuda.device_count()} GPU(s) to rank {rank}; "
                 f"run with --gpus <= {torch.cuda.device_count()} or on a node with {args.gpus} MI355X")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    numa = pin_to_gpu_numa_node(local_rank) if os.environ.get("STTM_BENCH_NO_PIN") != "1" else None
    dist = None
    if world > 1 or ("RANK" in os.environ and "MASTER_PORT" in os.environ):      # under torchrun (also with one rank)
        import torch.distributed as dist_mod
        dist = dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        assert dist.get_world_size() == args.gpus and dist.get_backend() == "nccl"

    from sttm_amd import _lib
    from sttm_amd.quadtree_interface import get_quadtree_features, get_quadtree_features_batch, quadtree_merge_raw
    from sttm_amd.synth import synth_video
    lib = _lib.load()

    T, C, H, W = args.frames, 1024, 14, 14
    thr, tthr, root = 0.85, 0.55, 1
    V, P, K, Wm = args.videos_per_step, max(1, args.pool), args.steps, args.warmup

    # ---- inputs: P distinct videos per GPU, generated on the device (same distribution as the CPU stream) ----
    pool = [synth_video(T, C, H, W, seed=100000 * (rank + 1) + i, device=dev, gen_device=dev) for i in range(P)]
    torch.cuda.synchronize()
    log(f"pool of {P} videos ready")

    last_call = [None]          # the results of the latest call of the step functions (what --dump-outputs writes)

    def run_step_dropin(s, sink):
        for v in range(V):
            x = pool[(s * V + v) % P]
            feat, npatch, tlbr = get_quadtree_features(x, thr, tthr, root)
            sink.append(feat.shape[0])
        last_call[0] = [(feat, npatch, tlbr)]

    BATCH = max(1, args.batch)

    # caller-owned output blocks for the batch entry point (ABI v8 `out=`): allocated ONCE, reused by every call -- what a pipeline that
    # consumes a call's results before issuing the next one does; no 10 GB of worst-case rows per call through the allocator
    out_blocks = None
    if args.mode == "batch" or (args.full and not args.no_extensions):
        nb_ = min(BATCH, V)
        out_blocks = (torch.empty((nb_, T * H * W, C), device=dev), torch.empty((nb_, T * H * W), dtype=torch.int32, device=dev),
                      torch.empty((nb_, T * H * W, 5), dtype=torch.int32, device=dev))

    def run_step_batch(s, sink):
        for b0 in range(0, V, BATCH):
            outs = get_quadtree_features_batch([pool[(s * V + v) % P] for v in range(b0, min(V, b0 + BATCH))], thr, tthr, root, out=out_blocks)
            sink.extend(o[0].shape[0] for o in outs)
        last_call[0] = outs

    def barrier():
        if dist is not None:
            dist.barrier(device_ids=[local_rank])

    # the rank logic (warm collectives, barrier + synchronise on both sides of exactly K timed steps, the job's one exchange step = the
    # gather of the per-video token counts, MAX over the ranks) lives in sttm_amd.distributed.run_sharded_job, which the world-size-2
    # gloo test drives with the CPU oracle as compute stand-in
    from sttm_amd.distributed import run_sharded_job
    step_fn = run_step_batch if args.mode == "batch" else run_step_dropin
    job = run_sharded_job(step_fn, K, Wm, V, rank, world, dev, dist, sync=torch.cuda, barrier_device_ids=[local_rank] if dist is not None else None)
    elapsed, videos, value, t_issue = job["elapsed_s"], job["videos"], job["value"], job["t_issue_s"]
    log(f"timed region ({args.mode}): {videos} videos in {elapsed:.4f} s = {value:.1f} videos/s (calls returned after {t_issue:.4f} s)")
    if args.dump_outputs and rank == 0:
        # before any other leg: the batch entry point's next call would overwrite the last call's results in out_blocks
        log(f"dumped outputs: {dump_outputs(args.dump_outputs, job['counts'][-V:], last_call[0])}")

    def timed(fn, n_videos):
        torch.cuda.synchronize()
        barrier()
        torch.cuda.synchronize()
        c0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        barrier()
        dt = time.perf_counter() - c0
        if dist is not None:
            tm = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(tm, op=dist.ReduceOp.MAX)
            dt = float(tm.item())
        return world * n_videos / dt

    # ---- validation mode: padded merged-token indices of a sample of videos to every rank ----------------
    validate = None
    if args.validate:
        from sttm_amd.distributed import gather_indices, shard_videos
        n_val = 4 * world
        ids_v = shard_videos(n_val, world, rank)
        loc = []
        # the CPU generator's many tiny ops crawl with one thread per core of a 128-core NUMA node (10 s per 16-frame clip,
        # 14 CPU-minutes for this leg): a handful of threads draws the same tensors in well under a second
        cpu_threads = torch.get_num_threads()
        torch.set_num_threads(min(cpu_threads, 8))
        for vid in ids_v:
            x = synth_video(T, C, H, W, seed=900000 + vid, device=dev)             # CPU generator: the same tensor on every rank
            _, _, tl = get_quadtree_features(x, thr, tthr, root)
            loc.append(tl[:, 0] * (H * W) + tl[:, 1] * W + tl[:, 2])
        full = gather_indices(ids_v, loc, n_val, T * H * W, dev, dist)
        # every rank recomputes ONE video it does not own and compares it with the gathered row
        other = (ids_v[-1] + 1) % n_val
        x = synth_video(T, C, H, W, seed=900000 + other, device=dev)
        _, _, tl = get_quadtree_features(x, thr, tthr, root)
        mine = (tl[:, 0] * (H * W) + tl[:, 1] * W + tl[:, 2]).to(torch.int32)
        row = full[other]
        ok = bool((row[:mine.numel()] == mine).all()) and bool((row[mine.numel():] == -1).all())
        okt = torch.tensor([1 if ok else 0], device=dev)
        if dist is not None:
            dist.all_reduce(okt, op=dist.ReduceOp.MIN)
        torch.set_num_threads(cpu_threads)
        validate = {"videos": n_val, "index_rows_gathered": int((full[:, 0] >= 0).sum()), "cross_rank_index_match": bool(okt.item())}
        log(f"validate: {validate}")

    # ---- extension legs (identical outputs; never the headline value) ---------------------------------------------------
    ext = {}
    if args.full and not args.no_extensions:
        KE = max(1, min(K, 4))
        # the mode the timed region did NOT run, same videos, KE steps
        if args.mode == "batch":
            sink2 = []
            run_step_dropin(0, sink2)
            dropin_vps = timed(lambda: [run_step_dropin(s_, sink2) for s_ in range(KE)], KE * V)
            ext["dropin_one_call_per_video"] = {
                "value": round(dropin_vps, 2), "unit": "videos/s",
                "frac": round((4 * C * T * H * W + (4 * C + 24) * (sum(sink2) / len(sink2))) * dropin_vps / world / 1e9 / HBM_PEAK_GBS, 4),
                "api": "get_quadtree_features, one video per call on one stream: the definition of `value` in rounds 1-4 (BENCH_r01..r04), "
                       "kept for a like-for-like comparison; a call's four dependent kernels and the host's wait for N' are serial here"}
            log(f"drop-in, one call per video, one stream: {dropin_vps:.1f} videos/s")
        else:
            sink2 = []
            run_step_batch(0, sink2)
            ext["batch_pipeline"] = {
                "value": round(timed(lambda: [run_step_batch(s_, sink2) for s_ in range(KE)], KE * V), 2), "unit": "videos/s",
                "api": f"get_quadtree_features_batch, {BATCH} videos per call over the library's internal streams (identical outputs)"}
            log(f"batch pipeline: {ext['batch_pipeline']['value']:.1f} videos/s")

        import threading
        NTH = 3

        def worker(k, n_steps):
            st = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(st):
                for s in range(n_steps):
                    for v in range(k, V, NTH):
                        get_quadtree_features(pool[(s * V + v) % P], thr, tthr, root)
            st.synchronize()

        def run_threads(n_steps):
            th = [threading.Thread(target=worker, args=(k, n_steps)) for k in range(NTH)]
            [t.start() for t in th]
            [t.join() for t in th]
        run_threads(1)
        ext["threaded_dropin_extension"] = {
            "value": round(timed(lambda: run_threads(KE), KE * V), 2), "unit": "videos/s",
            "api": "get_quadtree_features, one video per call, from 3 host threads with one stream each (identical outputs); the batch "
                   "entry point does the same overlap inside the library, without host threads"}
        log(f"threaded drop-in extension: {ext['threaded_dropin_extension']['value']:.1f} videos/s")

        # BASELINE config 5's other half: the ToMe baseline (tome_per_video, r = 0.5) on the same 128-frame clips; MFMA-bound
        from sttm_amd.tome_interface import get_tome_features
        NT = 32
        get_tome_features(pool[0], 0.5, "video")

        def run_tome():
            for v in range(NT):
                get_tome_features(pool[v % P], 0.5, "video")
        tome_vps = timed(run_tome, NT)
        n_tok = T * H * W
        flops = 2.0 * ((n_tok + 1) // 2) * (n_tok // 2) * C
        # the match computes every fp32 score from TOME_TERMS fp16 MFMA products (two-plane split, csrc/tome.hip; 3 by default since
        # round 5, 4 with tome_split = 1): the bound is the fp16 dense MFMA peak over that many instructions per fp32 product
        tome_peak = MFMA_F16_PEAK_TFLOPS / TOME_TERMS
        ext["tome_extension"] = {
            "value": round(tome_vps, 2), "unit": "videos/s", "config": f"ToMe video r=0.5, T={T} 14x14x1024 fp32",
            "roofline": {"bound": "mfma", "achieved": round(flops * tome_vps / world / 1e12, 2), "peak": tome_peak,
                         "unit": "TFLOP/s", "frac": round(flops * tome_vps / world / 1e12 / tome_peak, 4),
                         "flops_per_video": flops,
                         "x_fp32_mfma_peak": round(flops * tome_vps / world / 1e12 / MFMA_F32_PEAK_TFLOPS, 3),
                         "note": "whole get_tome_features call (normalise + match + sort + merge) over the match's ALGORITHMIC fp32 flops; "
                                 f"peak = 2500 TFLOP/s fp16 dense MFMA / {TOME_TERMS} product terms per fp32 score (rounds 2-4 ran 4 terms: bound 625); x_fp32_mfma_peak = the same rate "
                                 "over the 157.3 TFLOP/s fp32-input MFMA peak (round 1's kernel)"}}
        # the same clips as bfloat16 hidden states (what the reference's hook hands over in production): one bf16 MFMA per product
        xb = [pool[v % P].to(torch.bfloat16) for v in range(min(P, 4))]
        get_tome_features(xb[0], 0.5, "video")

        def run_tome_bf16():
            for v in range(NT):
                get_tome_features(xb[v % len(xb)], 0.5, "video")
        tome16_vps = timed(run_tome_bf16, NT)
        ext["tome_extension"]["bf16_inputs"] = {
            "value": round(tome16_vps, 2), "unit": "videos/s",
            "roofline": {"bound": "mfma", "achieved": round(flops * tome16_vps / world / 1e12, 2), "peak": MFMA_F16_PEAK_TFLOPS,
                         "unit": "TFLOP/s", "frac": round(flops * tome16_vps / world / 1e12 / MFMA_F16_PEAK_TFLOPS, 4)}}
        del xb
        log(f"tome extension: {tome_vps:.1f} videos/s = {ext['tome_extension']['roofline']['achieved']} TFLOP/s")

    # ---- hook leg: what the patched decoder forward does around the merge (quadtree_attn_monkey_patch.py:88-117) at the production
    #      shape: bf16 hidden states [1, 20 system + T*196 visual + 60 instruction tokens, 3584]; slice -> merge -> concat as the
    #      reference writes it (merge + torch.cat) against the fused form (the kernels write into the new hidden-state buffer) ----
    if args.full and not args.no_extensions:
        from sttm_amd import get_quadtree_features_into, patch_hooks
        Ch, n_sys, n_inst = 3584, 20, 60
        hs_pool = []
        for sidx in range(3):                              # 3 x 180 MB of hidden states: past the Infinity Cache
            vid = synth_video(T, Ch, H, W, seed=8000 + 10 * rank + sidx, dtype=torch.bfloat16, device=dev, gen_device=dev)
            vis = vid.permute(0, 2, 3, 1).reshape(1, T * H * W, Ch)
            hs_pool.append(torch.cat([torch.randn(1, n_sys, Ch, device=dev, dtype=torch.bfloat16), vis,
                                      torch.randn(1, n_inst, Ch, device=dev, dtype=torch.bfloat16)], 1).contiguous())
            del vid, vis
        pos = torch.arange(hs_pool[0].shape[1], device=dev).unsqueeze(0)
        hook = {}
        for label, into in (("merge_then_cat", None), ("fused_into_new_buffer", get_quadtree_features_into)):
            def run_hook(into=into, n=48):
                for it in range(n):
                    patch_hooks.quadtree_merge_llava(hs_pool[it % 3], pos, n_sys, T * H * W, T, get_quadtree_features, thr, tthr, root,
                                                     False, merge_into_fn=into)
            run_hook(n=6)
            hook[label + "_us_per_call"] = round(1e6 / (timed(run_hook, 48) / world), 1)
        hook["shape"] = f"hidden_states [1, {n_sys} + {T}*{H * W} + {n_inst}, {Ch}] bf16, STTM(0.85, 0.55, root 1)"
        hook["what"] = ("patch_hooks.quadtree_merge_llava = the reference hook's slice -> get_quadtree_features -> torch.cat -> index "
                        "arithmetic -> position-id truncation; fused = get_quadtree_features_into writes the merged rows straight into the "
                        "new hidden-state buffer (one copy of the system / instruction rows, none of the merged rows)")
        ext["hook_extension"] = hook
        log(f"hook extension: {hook['merge_then_cat_us_per_call']} us three-step, {hook['fused_into_new_buffer_us_per_call']} us fused")
        del hs_pool

    # ---- configs leg: every BASELINE.json configuration + the production shapes, drop-in API, a few hundred ms each --------
    configs = None
    if args.full and not args.no_configs:
        configs = run_configs(dev, rank, world, timed, log)

    roofline = None
    if args.full:
        # ---- roofline leg: per-kernel HIP events recorded by the library on the launch stream, a bounded number of calls ----
        ev = _lib.KernelEvents()
        tot = [0.0] * 4
        span = 0.0
        nodes = merged = leafnodes = 0
        calls = 0
        n_prof = max(8, min(args.profile_calls, K * V))
        for i in range(n_prof):
            x = pool[i % P]
            _, _, _, cnt, ctx = quadtree_merge_raw(x, thr, tthr, root, False, None, events=ev, return_ctx=True)
            ms = ev.elapsed_ms()                 # waits for the call's last event
            for k in range(4):
                tot[k] += ms[k]
            span += sum(ms)
            dcnt = ctx[2][0].tolist()            # the diagnostic counters live in device memory (complete once the call has drained)
            nodes += dcnt[_lib.CNT_NODES]
            leafnodes += dcnt[_lib.CNT_LEAFNODES]
            merged += cnt[_lib.CNT_OUT]
            calls += 1
        log("roofline leg done: " + ", ".join(f"{k}={t / calls:.4f} ms" for k, t in zip(KERNELS, tot)))
        avg_ms = [t / calls for t in tot]
        n_avg, m_avg, l_avg = nodes / calls, merged / calls, leafnodes / calls
        es = 4
        thw = T * H * W
        kernel_bytes = [                                     # algorithmic (compulsory) bytes of each kernel per launch
            es * C * thw + es * C * (n_avg - l_avg) + 24 * thw,   # read every token once, write every POOLED node once (1x1 nodes
                                                                  # stay in x), meta + inverse norm + default label / group size per token
            es * C * n_avg,                                   # every node row read once (pairs share rows)
            0.0,                                              # label kernel (k_col_labels): latency-bound, ~1 MB of edge lists and labels --
                                                              # it has no bandwidth roofline; its time is in kernel_ms
            es * C * n_avg + es * C * m_avg,                  # read node rows, write merged rows
        ]
        dom = max((0, 1, 3), key=lambda i: avg_ms[i])
        pipeline_bytes = es * C * thw + es * C * m_avg + 24 * m_avg      # B per video
        event_span_ms = span / calls                          # first event -> last event of a call WITH five event records in the stream:
                                                              # longer than the undisturbed call (the records sit between the kernels)
        wall_ms = elapsed / (K * V) * 1e3                     # the timed region itself: wall time per video on this GPU (includes the host)
        dom_gbs = kernel_bytes[dom] / (avg_ms[dom] * 1e-3) / 1e9
        pipe_gbs = pipeline_bytes / (wall_ms * 1e-3) / 1e9    # B over the time ONE video takes in the timed region
        # HBM traffic from the PMC counters: only if the committed passes were taken on THIS build of the library
        traffic = traffic_tag = traffic_where = None
        pmc_path = os.path.join(REPO, "profiles", "pmc_traffic.json")
        build_tag = _lib.build_tag()
        if os.path.exists(pmc_path):
            try:
                rec = json.load(open(pmc_path))
                if rec.get("workload") == f"T{T}_14x14x1024_f32_sttm_0.85_0.55" and rec.get("build_tag") == build_tag:
                    traffic = rec.get("hbm_bytes_per_video")
                    traffic_tag = rec.get("tag")
                    traffic_where = (f"an MI355X, profiles/{rec.get('tag')}_pmc_traffic.md, library build tag {rec.get('build_tag')} "
                                     "== the tag of the library loaded now; NOT re-measured during this run (PMC passes need rocprofv3)")
            except Exception:  # noqa: BLE001
                traffic = None
        roofline = {
            "bound": "hbm", "scope": "pipeline: the whole merge of one video (SURVEY 8d: B / wall time per video of the timed region, i.e. B * value / "
                                     "n_gpus); the dominant kernel's own figure is under dominant_kernel",
            "achieved": round(pipe_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(pipe_gbs / HBM_PEAK_GBS, 4),
            "frac_of_copy_rate": round(pipe_gbs / HBM_COPY_GBS, 4), "copy_rate_GBs": HBM_COPY_GBS,
            "traffic": traffic, "traffic_profile": traffic_tag, "traffic_measured_on": traffic_where, "build_tag": build_tag,
            "algorithmic_MB_per_video": round(pipeline_bytes / 1e6, 2), "wall_ms_per_video": round(wall_ms, 4),
            "event_span_ms_per_video": round(event_span_ms, 4),
            "dominant_kernel": {"kernel": KERNELS[dom], "achieved": round(dom_gbs, 1), "frac": round(dom_gbs / HBM_PEAK_GBS, 4),
                                "frac_of_copy_rate": round(dom_gbs / HBM_COPY_GBS, 4),
                                "algorithmic_MB": round(kernel_bytes[dom] / 1e6, 2), "ms": round(avg_ms[dom], 4)},
            "kernel_ms": {k: round(v, 4) for k, v in zip(KERNELS, avg_ms)},
            "kernel_ms_note": "HIP-event intervals recorded by the library on the launch stream during a separate leg; the event "
                              "records themselves add ~1-2 us per interval -- profiles/*_rocprofv3_kernel_stats.md holds the undisturbed durations",
            "kernel_algorithmic_MB": {k: round(b / 1e6, 2) for k, b in zip(KERNELS, kernel_bytes)},
            "profiled_calls": calls,
        }

    # ---- CPU baseline leg (rank 0, N = 1 only): the oracle on a bounded sample of the same workload -------
    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        from oracle import sttm_oracle as O
        host = host_cpu_facts()
        ncpu = host["logical_cpus"]          # (the CPUs this process may run on: what torch can use, and what cpu_baseline reports)
        # the pool the GPU path was timed on + 16 further distinct synth-v1 videos: 24 videos checked index-exact against the oracle
        n_extra = 16
        sample_dev = [pool[i] for i in range(min(P, 8))]
        sample_dev += [synth_video(T, C, H, W, seed=500000 + i, device=dev, gen_device=dev) for i in range(n_extra)]
        sample = [x.cpu() for x in sample_dev]
        # pick the thread count the CPU path likes best on this host (best case for the baseline)
        best_thr, best_t = None, None
        for nthr in sorted({min(ncpu, c) for c in (8, 16, 32, 64)}):
            torch.set_num_threads(nthr)
            O.get_quadtree_features(sample[0], thr, tthr, root)               # warm-up, untimed
            c0 = time.perf_counter()
            O.get_quadtree_features(sample[0], thr, tthr, root)
            dt = time.perf_counter() - c0
            log(f"cpu baseline: {nthr:3d} threads -> {dt * 1e3:.1f} ms / video")
            if best_t is None or dt < best_t:
                best_thr, best_t = nthr, dt
            if dt > 1.5 * best_t:
                break                                                          # more threads only get slower from here (128: 6 s per video)
        torch.set_num_threads(best_thr)
        done, match, spent = 0, 0, 0.0
        wall0 = time.perf_counter()
        while (spent < args.cpu_seconds or done < len(sample)) and done < 96 and time.perf_counter() - wall0 < 60.0:
            x = sample[done % len(sample)]
            c0 = time.perf_counter()
            ef, en, et = O.get_quadtree_features(x, thr, tthr, root)
            spent += time.perf_counter() - c0
            if done < len(sample):                                             # parity of the GPU path on the same input, both entry points
                f, n, t = get_quadtree_features(sample_dev[done], thr, tthr, root)
                if t.shape == et.shape and torch.equal(t.cpu(), et) and torch.equal(n.cpu(), en) \
                        and float((f.cpu() - ef).abs().max()) <= 1e-5:
                    match += 1
            done += 1
        checked = min(done, len(sample))
        # ... and the batch entry point (the timed region's mode) on the same 24 videos: bit-identical to the per-video calls
        bouts = get_quadtree_features_batch(sample_dev[:checked], thr, tthr, root)
        batch_same = sum(1 for x, (bf, bn, bt) in zip(sample_dev, bouts)
                         if all(torch.equal(a, b) for a, b in zip((bf, bn, bt), get_quadtree_features(x, thr, tthr, root))))
        log(f"cpu baseline: {done} videos in {spent:.2f} s with {best_thr} threads; {match}/{checked} index-exact; batch == per-video on {batch_same}/{checked}")
        del sample_dev
        cpu = {"value": round(done / spent, 3), "unit": "videos/s", "cores": best_thr, "threads": best_thr,
               "cores_meaning": "torch intra-op threads the oracle ran on (the bench contract's `cores` = threads actually used); the host's "
                                "physical core count is host_physical_cores",
               "host_logical_cpus": host["logical_cpus"], "host_physical_cores": host["physical_cores"], "host_cpu": host["model"],
               "kind": "port",
               "sample": f"{done} runs over {len(sample)} distinct synth-v1 videos (the GPU pool + {n_extra} more), T={T} 14x14x1024 fp32, "
                         f"STTM(0.85,0.55,root=1), oracle/sttm_oracle.py on torch CPU, best of 8/16/32/64 threads = {best_thr} "
                         f"(host has {ncpu} logical CPUs), 1 warm-up",
               "index_exact_videos": match, "videos_checked": checked, "batch_equals_per_video_calls": batch_same}

    if rank == 0:
        out = {
            "metric": "videos/sec (128-frame, 14x14x1024 tokens) STTM merge; merged-index match vs ref",
            "value": round(value, 2), "unit": "videos/s", "n_gpus": world, "steps": K, "warmup": Wm,
            # what `value` is (rounds 1-4: one video per call; since round 5 the batch entry point) and the other definition next to it,
            # at top level, so that no consumer compares numbers of different definitions
            "value_definition": ("batch entry point: get_quadtree_features_batch, %d independent videos per call (library-internal streams); "
                                 "NOT the definition of rounds 1-4 -- compare those with value_one_call_per_video" % BATCH) if args.mode == "batch"
                                else "one get_quadtree_features call per video on one stream (the reference's API; the definition of rounds 1-4)",
            "value_one_call_per_video": (ext.get("dropin_one_call_per_video", {}).get("value") if args.mode == "batch" else round(value, 2)),
            "value_batch_entry_point": (round(value, 2) if args.mode == "batch" else ext.get("batch_pipeline", {}).get("value")),
            "ms_per_step": round(elapsed / K * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"synth-v1 T={T} 14x14x1024 fp32, STTM spatial 0.85 + temporal 0.55, root_level 1",
                       "videos_per_step": V, "pool_per_gpu": P, "global_videos": videos, "parallelism": f"videos sharded x{world}",
                       "mode": args.mode,
                       "api": (f"get_quadtree_features_batch: {BATCH} independent videos per call -> sttm_quadtree_merge_batch deals them out to the "
                               "library's internal streams (whole per-video kernel chains, stage-skewed), written into caller-owned output blocks (out=, allocated once); every video's outputs incl. its host-visible "
                               "token count N' are produced, bit-identical to one call per video (tests/test_hip_parity.py::"
                               "test_batched_extension_equals_per_video_calls); the one-call-per-video rate of rounds 1-4 is under "
                               "dropin_one_call_per_video") if args.mode == "batch" else
                              "get_quadtree_features, one video per call (the reference's drop-in boundary)"},
            "roofline": roofline,
            "cpu_baseline": cpu,
        }
        out.update(ext)
        if configs is not None:
            out["configs"] = configs
        if numa is not None:
            out["host_affinity"] = numa
        if validate is not None:
            out["validate"] = validate
        if cpu:
            out["index_match"] = cpu["index_exact_videos"] / max(1, cpu["videos_checked"])
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
