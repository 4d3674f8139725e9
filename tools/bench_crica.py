#!/usr/bin/env python3
"""CricaVPR native branch: ms per keyframe at one batch size, the head alone and the 768-dim
default beside it, in one session on one GPU.

    python tools/bench_crica.py [--batch 64] [--group 1] [--repeats 5] [--out profiles/crica_head.json]

Times with HIP events, after warm-up, `--repeats` times each and interleaved:

  forward   CricaGPU.forward on `--batch` synthetic 640x480 keyframes (split-bf16 ViT-B/14 at
            322 x 322, the pyramid, the 2-layer cross-image encoder; 10752-dim);
  default   VitB14.forward (GeM, 768-dim): what CricaVPR runs without the opt-in;
  pool      the pyramid op alone on those frames' residual stream [batch, 530, 768];
  encoder   the encoder op alone on the pyramid rows [batch, 14, 768].

head = pool + encoder; head_share = head / forward.  By count the head is 0.31 GFLOP per frame
(14 rows x 2 layers x (2304 + 768 + 2048 + 2048) x 768 x 2, against the trunk's 100.9) but its
GEMMs have 14 rows per frame, so at small batches they stream the 44 MB of head weights
([W_hi | W_lo] bf16) once per call for little arithmetic.  Prints one JSON line (and writes it
to --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-level-indoor-slam_amd"))

HEAD_FLOP = 14 * 2 * (2304 + 768 + 2048 + 2048) * 768 * 2  # per frame
HEAD_WEIGHT_BYTES = 2 * (2304 + 768 + 2048 + 2048) * 768 * 2 * 2  # per call


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--group", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=2, help="calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from mlgate import _native, synthetic
    from mlgate.crica import CricaGPU
    from mlgate.weights import crica_state_dict

    dev = _native.require_device("cuda")
    B = args.batch
    seq = synthetic.make_sequence(B, places=max(4, B // 8), seed=5)
    frames = torch.from_numpy(synthetic.frames_host(seq, np.arange(B), h=480, w=640)).to(dev)
    eng = CricaGPU(crica_state_dict(0), device="cuda", max_batch=max(B, args.group), group=args.group)
    tokens = eng.trunk(frames)
    pooled = eng.pool(tokens)
    arms = {"forward": lambda: eng.forward(frames), "default": lambda: eng._vit.forward(frames),
            "pool": lambda: eng.pool(tokens), "encoder": lambda: eng.encode(pooled)}

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
            ms[k].append(timed(fn) / B)

    res = {"bench": "crica_head", "batch": B, "group": args.group, "size": [480, 640], "image_size": eng.image_size,
           "repeats": args.repeats, "inner": args.inner, "device": torch.cuda.get_device_name(0)}
    for k, v in ms.items():
        res[k] = {"ms_per_kf": [round(x, 5) for x in v], "median_ms_per_kf": round(statistics.median(v), 5)}
    med = {k: statistics.median(v) for k, v in ms.items()}
    head = med["pool"] + med["encoder"]
    res["head_ms_per_kf"] = round(head, 5)
    res["head_share_of_forward"] = round(head / med["forward"], 5)
    res["native_over_default"] = round(med["forward"] / med["default"], 4)
    res["native_minus_default_ms_per_kf"] = round(med["forward"] - med["default"], 5)
    res["encoder_TFLOPs"] = round(HEAD_FLOP / (med["encoder"] * 1e-3) / 1e12, 3)
    res["encoder_weight_GBps"] = round(HEAD_WEIGHT_BYTES / (med["encoder"] * B * 1e-3) / 1e9, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
