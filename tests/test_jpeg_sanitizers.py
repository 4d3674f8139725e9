"""Host sanitizer run of the JPEG coefficient decoder (sanitizer builds of the
native host code).  csrc/jpeg.cpp parses untrusted files, so it is rebuilt here with
-fsanitize=address,undefined into a stand-alone program (tests/native/jpeg_fuzz.cpp) and
fed the valid fixtures plus a seeded corpus of hostile ones: truncations, bit flips,
segment lengths pointing anywhere, frame headers with zero / huge dimensions and any
sampling factors, Huffman tables whose counts overflow 256 symbols or the code space,
table ids out of range, scans that reference undefined tables, restart intervals larger
than the image, restart markers out of sequence.  Every input must be decoded or rejected
without a sanitizer report, and every parameter record produced must fit
mlg_jpeg_coef_bytes.  Host-only: no GPU, nothing preloaded, no Python in the process."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "multi-level-indoor-slam_amd", "csrc", "jpeg.cpp")
DRIVER = os.path.join(ROOT, "tests", "native", "jpeg_fuzz.cpp")


def _segments(b):
    """[(marker, offset of FF, total length incl. the two marker bytes)] up to and including SOS."""
    out, o = [], 2
    while o + 4 <= len(b) and b[o] == 0xFF:
        m, n = b[o + 1], struct.unpack(">H", b[o + 2:o + 4])[0]
        out.append((m, o, 2 + n))
        o += 2 + n
        if m == 0xDA:
            break
    return out


def _find(b, marker):
    return [(o, n) for m, o, n in _segments(b) if m == marker]


def _corpus(rng):
    cases, _, _ = jpeg_ref.load_cases()
    good = [c["blob"] for c in cases if c["name"].startswith(("grid_37x53", "grid_17x31", "tiny_3x5", "tiny_9x1",
                                                              "dqt16", "optimize"))]
    good += [c["blob"] for c in cases if c["kind"] != "ok"]
    out = list(good)
    valid = [c["blob"] for c in cases if c["kind"] == "ok" and c["name"].startswith("grid_")]
    for it in range(160):
        b = bytearray(valid[int(rng.integers(0, len(valid)))])
        kind = it % 10
        if kind == 0:  # truncation
            b = b[:int(rng.integers(0, len(b)))]
        elif kind == 1:  # bit flips anywhere
            for _ in range(int(rng.integers(1, 8))):
                b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
        elif kind == 2:  # a segment length pointing anywhere
            segs = _segments(b)
            _, o, _ = segs[int(rng.integers(0, len(segs)))]
            b[o + 2:o + 4] = struct.pack(">H", int(rng.integers(0, 1 << 16)))
        elif kind == 3:  # frame header: zero / huge dimensions, sampling factors 0..15, table ids, precision
            (o, n), = _find(b, 0xC0)
            hh, ww = (int(rng.choice([0, 1, 7, 37, 65535])) for _ in range(2))
            b[o + 5:o + 9] = struct.pack(">HH", hh, ww)
            if rng.random() < 0.3:
                b[o + 4] = int(rng.choice([0, 8, 12, 16]))
            for c in range(b[o + 9]):
                if rng.random() < 0.7:
                    b[o + 11 + 3 * c] = int(rng.integers(0, 256))
                if rng.random() < 0.3:
                    b[o + 12 + 3 * c] = int(rng.integers(0, 256))
            if rng.random() < 0.3:
                b[o + 9] = int(rng.integers(0, 256))  # component count that disagrees with the length
        elif kind == 4:  # Huffman counts that overflow 256 symbols / the segment / the code space
            dht = _find(b, 0xC4)
            o, n = dht[int(rng.integers(0, len(dht)))]
            for l in range(16):
                if rng.random() < 0.4:
                    b[o + 5 + l] = int(rng.choice([0, 1, 17, 200, 255]))
        elif kind == 5:  # DQT / DHT ids and precision out of range
            segs = _find(b, 0xDB) + _find(b, 0xC4)
            o, n = segs[int(rng.integers(0, len(segs)))]
            b[o + 4] = int(rng.integers(0, 256))
        elif kind == 6:  # a scan that references tables never defined, or other components
            (o, n), = _find(b, 0xDA)
            for c in range(b[o + 4]):
                if rng.random() < 0.3:
                    b[o + 5 + 2 * c] = int(rng.integers(0, 256))
                b[o + 6 + 2 * c] = int(rng.choice([0x22, 0x33, 0x13, 0x30, 0xff, 0x44]))
        elif kind == 7:  # a restart interval larger than the image, or none where markers follow
            (o, n), = _find(b, 0xDD)
            b[o + 4:o + 6] = struct.pack(">H", int(rng.choice([0, 5, 1000, 65535])))
        elif kind == 8:  # restart markers out of sequence
            (so, sn), = _find(b, 0xDA)
            rst = [i for i in range(so + sn, len(b) - 1) if b[i] == 0xFF and 0xD0 <= b[i + 1] <= 0xD7]
            for i in rst:
                if rng.random() < 0.5:
                    b[i + 1] = 0xD0 + int(rng.integers(0, 8))
        else:  # entropy data replaced by noise (stuffed and unstuffed FFs, stray markers)
            (so, sn), = _find(b, 0xDA)
            noise = rng.integers(0, 256, len(b) - so - sn - 2, dtype=np.uint8)
            noise[rng.random(len(noise)) < 0.05] = 0xFF
            b[so + sn:len(b) - 2] = bytes(noise)
        out.append(bytes(b))
    out += [b"", b"\xff\xd8", b"\xff\xd8\xff", b"\xff\xd8" + b"\xff" * 40, b"\xff\xd8\xff\xc0\x00\x02"]
    return out, len(good)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_jpeg_decoder_under_asan_ubsan(tmp_path):
    exe = tmp_path / "jpeg_fuzz"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", SRC, DRIVER, "-o", str(exe), "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in r.stderr.lower():
        pytest.skip("AddressSanitizer runtime not available: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr
    corpus, ngood = _corpus(np.random.default_rng(4321))
    files = []
    for i, blob in enumerate(corpus):
        p = tmp_path / f"{i:04d}.jpg"
        p.write_bytes(blob)
        files.append(str(p))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)] + files, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    decoded, rejected = (int(x) for x in re.findall(r"\d+", r.stdout)[:2])
    assert decoded >= 20 and rejected >= 150
