"""DINOv2 ViT-S / B / L-14 forward rates on one MI355X (GPU box tool; no pass bar).

    python tools/bench_dino_backbones.py [--batch 64] [--size 322] [--reps 5] [--iters 20] [--out profiles/dino_backbones.json]

For each backbone and each packing (split: the MLG_VIT_SPLIT forward; bf16: the plain one) the
forward of one batch of bench.py-style synthetic keyframes through DinoVit.forward_into, with
the local features: one warm-up call, then `reps` windows of `iters` calls timed with HIP
events.  frames/s is reported as the median window with the min and max (the spread).  A
separate pass with the mlg_prof slots enabled (events around every GEMM and attention launch;
they add host work, so the end-to-end windows run without them) gives the achieved TFLOP/s of
qkv, proj, fc1, fc2 and attention: the algorithmic FLOPs of include/mlgate.h's shapes (for the
split forward three MFMA products per algorithmic product, as abi.cpp counts them) over the
summed event time of the slot.  ViT-S with the split packing also issues MFMAs on its zero
padding: `issued_over_algorithmic` is that ratio from the shapes (14 / 12 over a block's four
GEMMs), and `tflops_issued` the slot rates scaled by each GEMM's own ratio."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-level-indoor-slam_amd"))
sys.path.insert(0, ROOT)

from mlgate import _native, synthetic  # noqa: E402
from mlgate.vit import DinoVit  # noqa: E402
from mlgate.weights import BACKBONES, synthetic_state_dict  # noqa: E402

SLOTS = ((2, "qkv"), (3, "proj"), (0, "fc1"), (1, "fc2"), (4, "attention"))


def pad256(n):
    return (n + 255) // 256 * 256


def issued_ratios(E, split):
    """Per GEMM, columns the kernel runs over columns the network has (the split GEMM's 256-column tile)."""
    n = {"qkv": 3 * E, "proj": E, "fc1": 4 * E, "fc2": E}
    return {k: (pad256(v) / v if split else 1.0) for k, v in n.items()}


def block_ratio(E, split):
    """Issued over algorithmic MFMA products of a block's four GEMMs (N x K summed)."""
    k = {"qkv": E, "proj": E, "fc1": E, "fc2": 4 * E}
    n = {"qkv": 3 * E, "proj": E, "fc1": 4 * E, "fc2": E}
    r = issued_ratios(E, split)
    return sum(n[g] * r[g] * k[g] for g in n) / sum(n[g] * k[g] for g in n)


def measure(backbone, split, frames, a, L):
    E = BACKBONES[backbone][0]
    eng = DinoVit(synthetic_state_dict(0, backbone), backbone=backbone, device=frames.device, image_size=a.size,
                  max_batch=a.batch, precise=split)
    desc = torch.empty(len(frames), E, device=frames.device)
    local = torch.empty(len(frames), eng.n_local, E, device=frames.device)
    eng.forward_into(frames, desc, local)  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    fps = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            eng.forward_into(frames, desc, local)
        e1.record()
        torch.cuda.synchronize()
        fps.append(a.iters * len(frames) / (e0.elapsed_time(e1) * 1e-3))
    L.mlg_prof_reset()
    L.mlg_prof_enable(0x1F)
    for _ in range(a.iters):
        eng.forward_into(frames, desc, local)
    torch.cuda.synchronize()
    L.mlg_prof_enable(0)
    res = {"backbone": backbone, "packing": "split" if split else "bf16", "batch": len(frames), "image_size": a.size,
           "frames_per_s": {"median": round(statistics.median(fps), 1), "min": round(min(fps), 1),
                            "max": round(max(fps), 1), "windows": a.reps, "calls_per_window": a.iters},
           "issued_over_algorithmic": round(block_ratio(E, split), 4), "tflops": {}, "tflops_issued": {}}
    ratios = issued_ratios(E, split)
    for slot, name in SLOTS:
        ms, cnt, work = ctypes.c_double(), ctypes.c_long(), ctypes.c_double()
        L.mlg_prof_read(slot, ctypes.byref(ms), ctypes.byref(cnt))
        L.mlg_prof_read_work(slot, ctypes.byref(work))
        t = work.value / (ms.value * 1e9) if ms.value else None
        res["tflops"][name] = None if t is None else round(t, 1)
        res["tflops_issued"][name] = None if t is None else round(t * ratios.get(name, 1.0), 1)
    del eng, desc, local
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=322)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--backbones", default=",".join(BACKBONES))
    ap.add_argument("--out", default=None, help="also write the rows to this JSON file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dino_backbones: no HIP device (rates are measured on the GPU only)")
    dev = torch.device("cuda:0")
    seq = synthetic.make_sequence(a.batch, max(2, a.batch // 4), 0)
    frames = synthetic.frames_device(seq, np.arange(a.batch), dev)
    L = _native.lib()
    rows = []
    for backbone in a.backbones.split(","):
        for split in (True, False):
            rows.append(measure(backbone, split, frames, a, L))
            print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(dev), "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
