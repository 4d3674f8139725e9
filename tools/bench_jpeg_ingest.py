#!/usr/bin/env python3
"""JPEG keyframe ingestion rate: the native path against the reader it
replaces, in one session on one GPU.

    python tools/bench_jpeg_ingest.py [--frames 2000] [--repeats 3] [--out FILE]

Encodes `--frames` synthetic 640x480 keyframes (mlgate.synthetic) as JPEG with Pillow
(quality 90, 4:2:0; Pillow is needed for that and for the legacy arm -- the tool says so
and exits without it), then times, `--repeats` times each and interleaved:

  native  mlgate.ingest.KeyframeStream over the files at 16 host threads (Huffman decode
          on the pool, coefficients uploaded on a side stream, jpeg_pixels on the GPU);
  legacy  what process_image_sequence did per *.jpg file before: jpeg_reader()(path) on
          the calling thread, then a synchronous upload of the pageable array.

Both arms end with the frames in HBM and a device synchronisation; neither runs the ViT.
Also reports the jpeg_pixels kernel time per frame from HIP events.  Prints one JSON line
(and writes it to --out)."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-level-indoor-slam_amd"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--batch", type=int, default=123)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    try:
        from PIL import Image
    except ImportError:
        print("bench_jpeg_ingest: Pillow is required (it encodes the test frames and is the legacy reader); "
              "not installed, nothing measured")
        return 0
    import numpy as np
    import torch
    from mlgate import _native, ingest, synthetic

    dev = _native.require_device("cuda")
    H, W = 480, 640
    seq = synthetic.make_sequence(args.frames, places=max(4, args.frames // 8), seed=5)
    with tempfile.TemporaryDirectory() as tmp:
        paths, total = [], 0
        for lo in range(0, args.frames, 100):
            idx = np.arange(lo, min(args.frames, lo + 100))
            for i, fr in zip(idx, synthetic.frames_host(seq, idx, h=H, w=W)):
                f = io.BytesIO()
                Image.fromarray(np.ascontiguousarray(fr[..., ::-1])).save(f, "JPEG", quality=90, subsampling="4:2:0")
                p = os.path.join(tmp, f"{seq.t[i]:012.6f}.jpg")
                with open(p, "wb") as g:
                    g.write(f.getvalue())
                total += f.tell()
                paths.append(p)
        read = ingest.jpeg_reader()

        def native():
            n = 0
            t0 = time.perf_counter()
            for idx, frames in ingest.KeyframeStream(paths, device="cuda", batch=args.batch, threads=args.threads):
                n += frames.shape[0]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert n == len(paths)
            return dt

        def legacy():
            t0 = time.perf_counter()
            for p in paths:
                frame = torch.from_numpy(read(p)).to(dev)
            torch.cuda.synchronize()
            del frame
            return time.perf_counter() - t0

        # exactness of what is being timed, and a warm page cache / allocator for both arms
        idx, frames = next(iter(ingest.KeyframeStream(paths[:8], device="cuda", threads=args.threads)))
        for i, fr in zip(idx, frames.cpu().numpy()):
            assert np.array_equal(fr, read(paths[i])), "native pixels differ from the legacy reader's"
        native()
        times = {"native": [], "legacy": []}
        for _ in range(args.repeats):
            times["native"].append(native())
            times["legacy"].append(legacy())

        # kernel time per frame: one batch of coefficients in HBM, HIP events around repeated launches
        n = min(args.batch, len(paths))
        host = torch.empty(ingest._JpegStage.nbytes(n, H, W), dtype=torch.uint8, pin_memory=True)
        stage = ingest._JpegStage(host, n, H, W)
        st = ingest.load_jpeg_coefs(paths[:n], H, W, stage, args.threads)
        assert not st.any()
        buf = host[:stage.upload].to(dev)
        for _ in range(3):
            stage.pixels(buf)
        reps = 20
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            stage.pixels(buf)
        e1.record()
        torch.cuda.synchronize()
        kernel_us = e0.elapsed_time(e1) * 1e3 / (reps * n)
        t0 = time.perf_counter()
        ingest.load_jpeg_coefs(paths[:n], H, W, stage, args.threads)
        host_us = (time.perf_counter() - t0) * 1e6 / n

    def rate(ts):
        return [round(len(paths) / t, 1) for t in ts]

    res = {"bench": "jpeg_ingest", "frames": len(paths), "size": [H, W], "quality": 90, "subsampling": "4:2:0",
           "mean_file_bytes": round(total / len(paths)), "threads": args.threads, "batch": args.batch,
           "device": torch.cuda.get_device_name(0)}
    for k, ts in times.items():
        r = rate(ts)
        res[k] = {"kf_per_s": r, "median_kf_per_s": statistics.median(r), "spread_kf_per_s": round(max(r) - min(r), 1)}
    res["speedup_of_medians"] = round(res["native"]["median_kf_per_s"] / res["legacy"]["median_kf_per_s"], 2)
    # launch + record upload included (events around the op); traffic: coefficients read once
    # (3 B / pixel at 4:2:0) + the BGR store (3 B / pixel)
    res["jpeg_pixels_us_per_frame"] = round(kernel_us, 2)
    res["jpeg_pixels_GBps_at_6B_per_pixel"] = round(6 * H * W / kernel_us / 1e3, 1)
    res["host_huffman_us_per_frame_wall"] = round(host_us, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
