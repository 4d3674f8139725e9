"""JPEG keyframe ingestion on the GPU: host Huffman decode + the
``jpeg_pixels`` kernel (csrc/jpeg.hip: dequantise, jpeg_idct_islow, fancy upsampling,
YCbCr -> BGR) against the pixels libjpeg-turbo decodes from the same files
(tests/golden/jpeg_cases.npz).  Everything is integer arithmetic, so every comparison is
exact; only the descriptor comparison of process_image_sequence carries the 1e-6 that
tests/test_ingest_gpu.py sets for a device batch against one frame per call."""
import warnings

import numpy as np
import pytest
import torch

import jpeg_ref
import mlgate
from mlgate import _native, ingest
from mlgate.vpr import process_image_sequence

pytestmark = pytest.mark.gpu

CASES, SEQ_T, SEQ_FLOOR = jpeg_ref.load_cases()
OK = [c for c in CASES if c["kind"] == "ok"]
SEQ = [c for c in OK if c["name"].startswith("seq_")]


def test_decode_jpeg_bytes_equals_libjpeg_bit_for_bit(dev):
    """Every supported case, batched by frame size: subsamplings (and gray) mix inside a batch."""
    by_size = {}
    for c in OK:
        by_size.setdefault(c["bgr"].shape[:2], []).append(c)
    assert len(by_size) >= 5 + 36 + 1
    mixed = 0
    for (H, W), group in sorted(by_size.items()):
        frames, status = ingest.decode_jpeg_bytes([c["blob"] for c in group], H, W, device="cuda")
        assert frames.shape == (len(group), H, W, 3) and frames.dtype == torch.uint8 and frames.is_cuda
        assert not status.any(), [c["name"] for c, s in zip(group, status) if s]
        got = frames.cpu().numpy()
        for g, c in zip(got, group):
            assert np.array_equal(g, c["bgr"]), (c["name"], int(np.abs(g.astype(int) - c["bgr"]).max()))
        mixed += len({c["name"].split("_")[2] for c in group if c["name"].startswith(("grid_", "tiny_"))}) > 1
    assert mixed >= 5 + 36


def test_declined_images_in_a_batch_leave_the_others_exact(dev):
    group = [c for c in CASES if c["bgr"] is not None and c["bgr"].shape[:2] == (37, 53)]
    group += [c for c in CASES if c["kind"] == "corrupt"]
    frames, status = ingest.decode_jpeg_bytes([c["blob"] for c in group], 37, 53, device="cuda")
    got = frames.cpu().numpy()
    for g, s, c in zip(got, status, group):
        if c["kind"] == "ok":
            assert s == 0 and np.array_equal(g, c["bgr"]), c["name"]
        else:
            assert s == (jpeg_ref.EUNSUP if c["kind"] == "unsupported" else jpeg_ref.EINVAL) and not g.any(), c["name"]


def test_keyframe_stream_mixes_png_jpeg_and_declined_files(dev, tmp_path):
    """PNG, native JPEG, broken files and a progressive JPEG (legacy reader), interleaved by
    name: exact frames in path order, the reference's warning for each broken file."""
    from test_ingest_cpu import encode_png
    want = []
    for i, c in enumerate(SEQ[:6]):
        if i % 3 == 0:
            (tmp_path / f"{i:02d}.png").write_bytes(encode_png(np.ascontiguousarray(c["bgr"][..., ::-1]), 2))
            want.append((f"{i:02d}.png", c["bgr"]))
        else:
            (tmp_path / f"{i:02d}.jpg").write_bytes(c["blob"])
            want.append((f"{i:02d}.jpg", c["bgr"]))
    small = next(c for c in OK if c["name"].startswith("grid_37x53_422"))  # another size: a batch of its own
    (tmp_path / "02b.jpeg").write_bytes(small["blob"])
    want.append(("02b.jpeg", small["bgr"]))
    (tmp_path / "04b.jpg").write_bytes(b"\xff\xd8 nope")            # no header: never reaches a batch
    (tmp_path / "01b.jpg").write_bytes(SEQ[1]["blob"][:len(SEQ[1]["blob"]) // 2])  # fails inside its batch
    bad = ["01b.jpg", "04b.jpg"]
    paths = sorted(tmp_path.iterdir())
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = []
        for idx, fr in ingest.KeyframeStream(paths, device="cuda", batch=4):
            assert fr.device.type == "cuda" and fr.dtype == torch.uint8 and fr.shape[0] == len(idx)
            got.extend(zip(idx, fr.cpu().numpy()))
    names = [p.name for p in paths]
    expect = sorted(want)
    assert [names[i] for i, _ in got] == [n for n, _ in expect]
    for (i, f), (n, px) in zip(got, expect):
        assert np.array_equal(f, px), n
    msgs = [str(x.message) for x in w if "Failed to load image" in str(x.message)]
    assert len(msgs) == len(bad) and all(n in m for n, m in zip(bad, msgs))

    # a valid stream the native path declines: the legacy reader's pixels, at its position
    pytest.importorskip("PIL.Image")
    prog = next(c for c in CASES if c["name"].startswith("progressive"))
    sub = tmp_path / "prog"
    sub.mkdir()
    (sub / "a.jpg").write_bytes(small["blob"])
    (sub / "b.jpg").write_bytes(prog["blob"])
    (sub / "c.jpg").write_bytes(small["blob"])
    out = [(idx, fr.cpu().numpy()) for idx, fr in ingest.KeyframeStream(sorted(sub.iterdir()), device="cuda")]
    assert [i for idx, _ in out for i in idx] == [0, 1, 2]
    flat = [f for _, fr in out for f in fr]
    assert np.array_equal(flat[0], small["bgr"]) and np.array_equal(flat[2], small["bgr"])
    assert np.array_equal(flat[1], prog["bgr"])


def test_process_image_sequence_jpeg_matches_reference_loop(dev, tmp_path):
    n = len(SEQ)
    t = 100.0 + SEQ_T * 15.0  # spread so min_time_gap 10 s admits revisits
    floors = SEQ_FLOOR
    for c, ti in zip(SEQ, t):
        (tmp_path / f"{ti:.6f}.jpg").write_bytes(c["blob"])
    order = sorted(range(n), key=lambda i: f"{t[i]:.6f}.jpg")
    # the reference pairs the i-th sorted file with the i-th timestamp
    spr, matches = process_image_sequence(tmp_path, t, floors, vpr_method="cricavpr", device="cuda")

    ref = mlgate.SemanticPlaceRecognition(vpr_method="cricavpr", device="cuda")
    for k, i in enumerate(order):
        ref.add_image(image=np.array(SEQ[i]["bgr"]), timestamp=t[k], floor_label=int(floors[k]),
                      image_path=str(tmp_path / f"{t[i]:.6f}.jpg"))
    ref_matches = ref.find_loop_closures(enable_floor_gating=True)
    a, b = spr.vpr.descriptors, ref.vpr.descriptors
    assert len(a) == len(b) == n
    for x, y in zip(a, b):
        assert x.timestamp == y.timestamp and x.floor_label == y.floor_label and x.image_path == y.image_path
        # device batch vs one frame per call: same kernels, tiles of another M
        assert np.allclose(x.descriptor, y.descriptor, rtol=0, atol=1e-6)
    assert [(m.query_idx, m.match_idx, m.is_valid) for m in matches] == \
           [(m.query_idx, m.match_idx, m.is_valid) for m in ref_matches]


def test_record_pointing_past_the_buffer_raises_before_launch(dev):
    c = next(c for c in OK if c["name"].startswith("grid_48x64_420"))
    ops = _native.ops()
    per = ops.jpeg_coef_bytes(48, 64)
    coefs = torch.zeros(per // 2, dtype=torch.int16)
    qtabs = torch.zeros((1, 3, 64), dtype=torch.uint16)
    params = torch.zeros((1, 16), dtype=torch.int32)
    st = ops.jpeg_coefs_decode([torch.frombuffer(bytearray(c["blob"]), dtype=torch.uint8)], coefs, qtabs, params,
                               48, 64, 1)
    assert st[0] == 0
    dc, dq = coefs.cuda(), qtabs.cuda()
    good = ops.jpeg_pixels(dc, dq, params, 48, 64)
    assert np.array_equal(good[0].cpu().numpy(), c["bgr"])
    assert np.array_equal(ops.jpeg_pixels(dc, dq, params.cuda(), 48, 64)[0].cpu().numpy(), c["bgr"])
    for pos, val in [(14, per // 2), (6, -64), (4, 1000), (0, 7), (1, 4)]:
        p = params.clone()
        p[0, pos] = val
        for q in (p, p.cuda()):
            with pytest.raises(RuntimeError, match="parameter records"):
                ops.jpeg_pixels(dc, dq, q, 48, 64)
    with pytest.raises(RuntimeError, match="coefs: needs"):
        ops.jpeg_pixels(dc[:-64], dq, params, 48, 64)
    torch.cuda.synchronize()
