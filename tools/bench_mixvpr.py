#!/usr/bin/env python3
"""MixVPR native branch: ms per keyframe at one batch size, split into its stages, with the
GAP fallback beside it, in one session on one GPU.

    python tools/bench_mixvpr.py [--batch 64] [--repeats 5] [--out profiles/mixvpr_native.json]

Times with HIP events, after warm-up, `--repeats` times each and interleaved:

  forward     MixVprGPU.forward on `--batch` synthetic 640x480 keyframes (preprocess, cropped
              ResNet-50 at 320 x 320, fused mixer head);
  preprocess  the preprocessing op alone;
  head        the head op alone on seeded post-ReLU features [batch, 400, 1024];
  fallback    ResNet50GPU.forward_device (the 224 x 224 GAP descriptor MixVPR runs by default).

trunk = forward - preprocess - head (derived, not timed on its own).  The head's rate is its
algorithmic work, 4 blocks x 2 Linear(400, 400) x 1024 rows = 2.62 GFLOP per frame plus the
8.4 MFLOP folded projection, over its time, against the 2.5 PFLOP/s dense bf16 peak; the same
time against the weight stream every 64-row tile re-reads from L2 (2.77 MB) is printed
beside it.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-level-indoor-slam_amd"))

BF16_PEAK = 2.5e15                               # dense bf16 MFMA, FLOP/s
HEAD_FLOP = 4 * 2 * 2 * 1024 * 400 * 400 + 2 * 4 * 1024 * (400 + 1024)  # per frame
TILE_WEIGHT_BYTES = 8 * 26 * 416 * 16 * 2        # bf16 weights one 64-row tile streams from L2


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=4, help="calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from mlgate import _native, synthetic
    from mlgate.mixvpr import MixVprGPU
    from mlgate.resnet import ResNet50GPU
    from mlgate.weights import mixvpr_state_dict

    dev = _native.require_device("cuda")
    B = args.batch
    seq = synthetic.make_sequence(B, places=max(4, B // 8), seed=5)
    frames = torch.from_numpy(synthetic.frames_host(seq, np.arange(B), h=480, w=640)).to(dev)
    rng = np.random.default_rng(5)
    feat = torch.from_numpy(np.maximum(rng.standard_normal((B, 400, 1024), dtype=np.float32), 0)).to(dev)
    eng = MixVprGPU(mixvpr_state_dict(0), device="cuda", max_batch=B)
    gap = ResNet50GPU(device="cuda")
    arms = {"forward": lambda: eng.forward(frames), "preprocess": lambda: eng.preprocess(frames),
            "head": lambda: eng.head(feat), "fallback": lambda: gap.forward_device(frames, 4096)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (args.inner * B)  # ms per keyframe

    for fn in arms.values():  # warm-up: code objects, allocator
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(args.repeats):
        for k, fn in arms.items():
            ms[k].append(timed(fn))

    res = {"bench": "mixvpr_native", "batch": B, "size": [480, 640], "repeats": args.repeats, "inner": args.inner,
           "device": torch.cuda.get_device_name(0)}
    for k, v in ms.items():
        res[k] = {"ms_per_kf": [round(x, 4) for x in v], "median_ms_per_kf": round(statistics.median(v), 4)}
    med = {k: statistics.median(v) for k, v in ms.items()}
    res["trunk_ms_per_kf_derived"] = round(med["forward"] - med["preprocess"] - med["head"], 4)
    head_s = med["head"] * 1e-3
    res["head_TFLOPs"] = round(HEAD_FLOP / head_s / 1e12, 1)
    res["head_frac_of_bf16_peak"] = round(HEAD_FLOP / head_s / BF16_PEAK, 4)
    res["head_L2_weight_stream_TBps"] = round(16 * TILE_WEIGHT_BYTES / head_s / 1e12, 2)  # 16 tiles per frame
    res["native_over_fallback"] = round(med["forward"] / med["fallback"], 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
