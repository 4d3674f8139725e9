"""JPEG keyframe ingestion, host half (csrc/jpeg.cpp): marker parse + Huffman
decode to quantised DCT coefficients, checked without a GPU.

The coefficients of every supported fixture (tests/golden/jpeg_cases.npz: file bytes and
the pixels Pillow's libjpeg-turbo decodes from them) are run through the numpy
restatement of the device half (tests/jpeg_ref.py) and must give libjpeg-turbo's pixels
bit for bit -- no tolerance.  Unsupported and damaged streams must get their status, and
the parameter-record check that guards the kernel's indexing is exercised through the C
ABI."""
import ctypes

import numpy as np
import pytest
import torch

import jpeg_ref
from jpeg_ref import EINVAL, ESIZE, EUNSUP
from mlgate import _native, ingest

CASES, _, _ = jpeg_ref.load_cases()
OK = [c for c in CASES if c["kind"] == "ok"]


def _decode(blobs, H, W, threads=1):
    """jpeg_coefs_decode -> (coefs int16 [n, per/2], qtabs uint16 [n, 3, 64], params int32 [n, 16], status)"""
    ops = _native.ops()
    n = len(blobs)
    per = ops.jpeg_coef_bytes(H, W)
    coefs = torch.full((n, per // 2), 0x5a5a, dtype=torch.int16)  # the decoder must zero-fill what it uses
    qtabs = torch.zeros((n, 3, 64), dtype=torch.uint16)
    params = torch.full((n, 16), -7, dtype=torch.int32)
    ts = [torch.frombuffer(bytearray(b), dtype=torch.uint8) if len(b) else torch.zeros(0, dtype=torch.uint8)
          for b in blobs]
    st = ops.jpeg_coefs_decode(ts, coefs, qtabs, params, H, W, threads)
    return coefs.numpy(), qtabs.numpy(), params.numpy(), st.numpy()


def test_fixture_covers_what_it_should():
    names = [c["name"] for c in OK]
    grid = [n for n in names if n.startswith("grid_")]
    assert len(grid) == 60 and all("_r" in n for n in grid)
    assert sum(n.startswith("tiny_") for n in names) == 108 and sum(n.startswith("seq_") for n in names) == 12
    assert any(n.startswith("dqt16") for n in names) and any(n.startswith("optimize") for n in names)
    assert sorted(c["name"].split("_")[0] for c in CASES if c["kind"] == "unsupported") == ["cmyk", "exif6", "progressive"]
    assert sorted(c["name"].split("_")[0] for c in CASES if c["kind"] == "corrupt") == ["badcode", "nope", "truncated"]


@pytest.mark.parametrize("prefix", ["grid_16x16", "grid_17x31", "grid_37x53", "grid_41x35", "grid_48x64", "tiny_",
                                    "dqt16", "optimize", "seq_"])
def test_coefficients_give_libjpeg_pixels_bit_for_bit(prefix):
    group = [c for c in OK if c["name"].startswith(prefix)]
    assert group
    for c in group:
        H, W = c["bgr"].shape[:2]
        coefs, qtabs, params, st = _decode([c["blob"]], H, W)
        assert st[0] == 0, c["name"]
        per = coefs.shape[1] * 2
        assert _native.lib().mlg_jpeg_params_check(params.ctypes.data, 1, H, W, per) == 0, c["name"]
        got = jpeg_ref.pixels(coefs[0], qtabs[0], params[0], H, W)
        assert np.array_equal(got, c["bgr"]), (c["name"], int(np.abs(got.astype(int) - c["bgr"]).max()))


def test_sixteen_bit_tables_are_kept_whole():
    c = next(c for c in OK if c["name"].startswith("dqt16"))
    H, W = c["bgr"].shape[:2]
    _, qtabs, _, st = _decode([c["blob"]], H, W)
    assert st[0] == 0 and qtabs.max() > 255


def test_status_of_unsupported_and_damaged_streams():
    for c in CASES:
        if c["kind"] == "ok":
            continue
        H, W = c["bgr"].shape[:2] if c["bgr"] is not None else (37, 53)
        _, _, params, st = _decode([c["blob"]], H, W)
        assert st[0] == (EUNSUP if c["kind"] == "unsupported" else EINVAL), (c["name"], st[0])
        assert not params.any()  # an undecoded image leaves an empty record
    c = next(c for c in OK if c["name"].startswith("grid_37x53_420"))
    assert _decode([c["blob"]], 37, 54)[3][0] == ESIZE
    assert _decode([c["blob"]], 53, 37)[3][0] == ESIZE
    assert _decode([b""], 8, 8)[3][0] == EINVAL


def test_jpeg_info_fields():
    want_sub = {"444": (3, 1, 1), "422": (3, 2, 1), "420": (3, 2, 2), "gray": (1, 1, 1)}
    for c in OK:
        if not c["name"].startswith("grid_"):
            continue
        H, W = c["bgr"].shape[:2]
        sub = c["name"].split("_")[2]
        assert ingest.jpeg_info(c["blob"]) == (W, H) + want_sub[sub] + (True,), c["name"]
    for c in CASES:
        if c["kind"] == "unsupported":
            info = ingest.jpeg_info(c["blob"])
            assert info[:2] == (53, 37) and info[5] is False, c["name"]
    assert ingest.jpeg_info(b"\xff\xd8 nope") is None
    assert ingest.jpeg_info(b"") is None
    # the header alone is enough: nothing after SOS is read
    c = next(c for c in OK if c["name"].startswith("seq_00"))
    sos = c["blob"].index(b"\xff\xda")
    assert ingest.jpeg_info(c["blob"][:sos + 14]) == (128, 96, 3, 2, 2, True)


def test_thread_count_does_not_change_the_buffers():
    group = [c for c in CASES if c["bgr"] is not None and c["bgr"].shape[:2] == (37, 53)]
    group += [c for c in CASES if c["kind"] == "corrupt"]
    blobs = [c["blob"] for c in group] * 3
    a = _decode(blobs, 37, 53, threads=1)
    b = _decode(blobs, 37, 53, threads=16)
    assert 0 in a[3] and EINVAL in a[3] and EUNSUP in a[3]
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_load_from_paths_equals_decode_from_memory(tmp_path):
    group = [c for c in OK if c["name"].startswith("seq_")][:4]
    paths = []
    for c in group:
        p = tmp_path / (c["name"] + ".jpg")
        p.write_bytes(c["blob"])
        paths.append(str(p))
    paths.append(str(tmp_path / "missing.jpg"))
    ops = _native.ops()
    n, per = len(paths), ops.jpeg_coef_bytes(96, 128)
    coefs = torch.zeros((n, per // 2), dtype=torch.int16)
    qtabs = torch.zeros((n, 3, 64), dtype=torch.uint16)
    params = torch.zeros((n, 16), dtype=torch.int32)
    st = ops.jpeg_coefs_load_into(paths, coefs, qtabs, params, 96, 128, 4).numpy()
    assert st.tolist() == [0, 0, 0, 0, EINVAL]
    mem = _decode([c["blob"] for c in group], 96, 128)
    used = int(params[0, 6 + 8]) + int(params[0, 4 + 8]) * int(params[0, 5 + 8]) * 64
    assert np.array_equal(coefs.numpy()[:4, :used], mem[0][:, :used])
    assert np.array_equal(qtabs.numpy()[:4], mem[1]) and np.array_equal(params.numpy()[:4], mem[2])
    with pytest.raises(RuntimeError, match="coefs: needs"):
        ops.jpeg_coefs_load_into(paths, coefs[:2], qtabs, params, 96, 128, 1)


def test_coef_bytes_is_the_worst_case_over_samplings():
    ops = _native.ops()
    for H, W in [(1, 1), (17, 31), (96, 128), (480, 640), (9, 9)]:
        b8 = lambda v: -(-v // 8)
        b16 = lambda v: 2 * -(-v // 16)
        want = max(3 * b8(H) * b8(W), b8(H) * b16(W) + 2 * b8(H) * (b16(W) // 2),
                   b16(H) * b16(W) + 2 * (b16(H) // 2) * (b16(W) // 2)) * 128
        assert ops.jpeg_coef_bytes(H, W) == want
    assert ops.jpeg_coef_bytes(0, 5) == 0 and ops.jpeg_coef_bytes(5, 70000) == 0


def test_parameter_records_are_validated_against_the_buffer():
    """What jpeg_pixels runs on every record before it launches (mlg_jpeg_params_check):
    the kernel indexes the coefficient buffer through the record alone."""
    check = _native.lib().mlg_jpeg_params_check
    c = next(c for c in OK if c["name"].startswith("grid_37x53_420"))
    coefs, _, params, st = _decode([c["blob"]], 37, 53)
    per = coefs.shape[1] * 2

    def rc(p, H=37, W=53, size=per):
        p = np.ascontiguousarray(p, dtype=np.int32)
        return check(p.ctypes.data_as(ctypes.c_void_p), p.size // 16, H, W, size)

    assert st[0] == 0 and rc(params) == 0
    assert rc(np.zeros((2, 16), np.int32)) == 0  # empty records: images that were not decoded
    bad = []
    for pos, val in [(0, 2), (0, 4), (0, -1), (1, 3), (1, 0), (2, 3), (2, 0), (4, params[0, 4] + 1),
                     (5, params[0, 5] - 1), (9, 0), (6, -64), (6, 32), (14, per // 2), (14, 2 ** 31 - 64),
                     (10, per // 2 - 64)]:
        p = params.copy()
        p[0, pos] = val
        bad.append(p)
    for p in bad:
        assert rc(p) == EINVAL, p
    used = int(params[0, 14]) + int(params[0, 12]) * int(params[0, 13]) * 64
    assert rc(params, size=2 * used) == 0 and rc(params, size=2 * used - 2) == EINVAL
    assert rc(params, H=38, W=53) == 0 and rc(params, H=49, W=53) == EINVAL  # another block count
    assert rc(params, H=0) == EINVAL and rc(params, W=70000) == EINVAL
    gray = params.copy()
    gray[0, 0] = 1  # one component cannot be subsampled
    assert rc(gray) == EINVAL


def test_jpeg_pixels_has_no_host_kernel():
    """The device half exists for HIP tensors only: host tensors fail loudly."""
    c = next(c for c in OK if c["name"].startswith("grid_16x16_444"))
    coefs, qtabs, params, _ = _decode([c["blob"]], 16, 16)
    with pytest.raises((NotImplementedError, RuntimeError)):
        _native.ops().jpeg_pixels(torch.from_numpy(coefs), torch.from_numpy(qtabs), torch.from_numpy(params), 16, 16)
