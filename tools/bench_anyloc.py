#!/usr/bin/env python3
"""AnyLoc native branch: ms per keyframe at one batch size, the VLAD head alone, the
mean-pool default beside it, and one k-means iteration of the vocabulary fit (DESIGN.md
row a7), in one session on one GPU.

    python tools/bench_anyloc.py [--batch 64] [--repeats 5] [--out profiles/anyloc_vlad.json]

Times with HIP events, after warm-up, `--repeats` times each and interleaved:

  forward   AnyLocGPU.forward on `--batch` synthetic 640x480 keyframes (split-bf16 ViT-B/14 at
            518 x 518, final norm, VLAD head; K = 64);
  head      the VLAD op alone on those frames' tokens [batch, 1368, 768];
  default   VitB14.forward with mean pooling: what AnyLoc runs without the opt-in;
  kmeans    one Lloyd iteration (torch.ops.mlgate.kmeans_step) over all batch x 1368 tokens,
            reported per call, not per keyframe.

The vocabulary is fitted on the same tokens (10 Lloyd steps), so the head sees the cluster
sizes a fitted vocabulary gives.  head_share = head / forward.  The head's algorithmic work
is the assignment GEMM, 2 x 1368 x 64 x 768 = 135 MFLOP per frame, on the exact-f32 MFMA
(157 TFLOP/s dense peak: 256 FLOP per cycle per CU, 256 CUs, 2.4 GHz), plus one read of the tokens
per pass (4.2 MB per frame, twice).  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-level-indoor-slam_amd"))

F32_MFMA_PEAK = 256 * 256 * 2.4e9  # FLOP/s
TOKENS, EMBED, K = 1368, 768, 64
ASSIGN_FLOP = 2 * TOKENS * K * EMBED  # per frame


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=2, help="calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from mlgate import _native, synthetic
    from mlgate.anyloc import AnyLocGPU, fit_vocabulary
    from mlgate.weights import synthetic_state_dict, synthetic_vocabulary

    dev = _native.require_device("cuda")
    B = args.batch
    seq = synthetic.make_sequence(B, places=max(4, B // 8), seed=5)
    frames = torch.from_numpy(synthetic.frames_host(seq, np.arange(B), h=480, w=640)).to(dev)
    eng = AnyLocGPU(synthetic_state_dict(0), synthetic_vocabulary(K), device="cuda", max_batch=B)
    tokens = eng.tokens(frames)
    flat = tokens.reshape(-1, EMBED)
    centers, info = fit_vocabulary(flat, K, seed=0, max_iter=10, return_info=True)
    eng.set_vocabulary(centers)
    km_centers = eng.centers.clone()
    km_labels = torch.from_numpy(info["labels"]).to(dev)
    ops = _native.ops()
    arms = {"forward": lambda: eng.forward(frames), "head": lambda: eng.vlad(tokens),
            "default": lambda: eng._vit.forward(frames),
            "kmeans": lambda: ops.kmeans_step(flat, km_centers, km_labels)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.inner  # ms per call

    for fn in arms.values():  # warm-up: code objects, allocator
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(args.repeats):
        for k, fn in arms.items():
            ms[k].append(timed(fn) / (1 if k == "kmeans" else B))

    res = {"bench": "anyloc_vlad", "batch": B, "size": [480, 640], "tokens": TOKENS, "clusters": K,
           "repeats": args.repeats, "inner": args.inner, "device": torch.cuda.get_device_name(0),
           "cluster_sizes_min_max": [int(info["counts"].min()), int(info["counts"].max())],
           # the longest in-order sum one workgroup of the aggregation carries
           "largest_cluster_in_one_frame": int(max(np.bincount(row, minlength=K).max()
                                                   for row in info["labels"].reshape(B, TOKENS)))}
    for k, v in ms.items():
        unit = "ms_per_call" if k == "kmeans" else "ms_per_kf"
        res[k] = {unit: [round(x, 5) for x in v], "median_" + unit: round(statistics.median(v), 5)}
    med = {k: statistics.median(v) for k, v in ms.items()}
    res["kmeans"]["tokens"] = B * TOKENS
    res["head_share_of_forward"] = round(med["head"] / med["forward"], 5)
    res["native_over_default"] = round(med["forward"] / med["default"], 4)
    res["head_assign_TFLOPs"] = round(ASSIGN_FLOP / (med["head"] * 1e-3) / 1e12, 2)
    res["head_frac_of_f32_mfma_peak"] = round(ASSIGN_FLOP / (med["head"] * 1e-3) / F32_MFMA_PEAK, 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
