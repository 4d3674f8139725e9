"""Every exported workspace size query returns what it returned before the carving was
moved into csrc/ws_carve.h (CPU only: libmlgate.so loads without a GPU).

Callers size their allocations from these values (mlgate/pipeline.py picks LightGlue's
chunk sizes from them), so a refactor of the host-side layouts must not move one byte.
tests/golden/workspace_sizes.json maps "function(args)" to bytes.  It was recorded by this
module's own record mode (`python tests/test_workspace_sizes_cpu.py --record`) at the
commit BEFORE the carving refactor touched any source, and is re-recorded only when a
layout changes on purpose.  The arguments are the smallest shapes at which a layout can
go wrong (tile and capacity thresholds, odd sizes, both arms of every branch, the
arguments each query refuses with 0) plus the workload's own.

mlg_proximity_workspace_bytes is not in the table: it includes rocprim's temporary-storage
query, which answers differently without a device (measured at that commit and after the
refactor alike: (N, nrows) = (0, 0) gives 256 bytes without a GPU and 1280 on an MI355X,
(5000, 5000) 240384 and 241408), so a value recorded on the CPU would not be the one
callers get.  tests/test_proximity_gpu.py covers it where it runs."""
import ctypes
import json
import os
import struct
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")


def _orb_params(H, W, nfeatures):
    """A host mlg_orb_params for an H x W frame: head, then the blocks mlgate.orb.geometry computes."""
    from mlgate import orb
    ip, fp = orb.geometry(H, W, nfeatures)
    body = struct.pack("<24i8f16i7f2i", *ip[:24].tolist(), *fp[:8].tolist(), *ip[24:40].tolist(), *fp[8:15].tolist(),
                       *ip[40:42].tolist())
    return ctypes.create_string_buffer(struct.pack("<II", 8 + len(body), 3) + body)


def _cases():
    """(key, function name, argument tuple); ORB's first argument is built per case."""
    c = []

    def add(fn, *args):
        c.append((f"{fn}({', '.join(str(a) for a in args)})", fn, args))

    for fn in ("mlg_lightglue_workspace_bytes", "mlg_superglue_workspace_bytes"):
        for kmax in (1, 63, 64, 65, 2048, 2049):
            add(fn, 1, kmax)
        for P in (64, 65, 0):  # the assignment capacity is min(P, 64)
            add(fn, P, 2048)
        add(fn, 3, 96)
        add(fn, 1, 0)
    # LoFTR match: csplit in its own region (2 P L < 128), aliased, the pair-group boundary
    for P, H, W in ((1, 32, 32), (2, 32, 32), (3, 32, 32), (4, 32, 32), (1, 64, 64), (8, 64, 64), (9, 64, 64),
                    (1, 480, 640), (2, 480, 640), (1, 536, 720), (1, 36, 32), (1, 32, 36), (1, 24, 32), (0, 32, 32)):
        add("mlg_loftr_match_ws_bytes", P, H, W)
    for B, H, W in ((1, 32, 32), (1, 36, 37), (2, 480, 640), (1, 540, 720), (1, 31, 32), (0, 32, 32)):
        add("mlg_loftr_features_ws_bytes", B, H, W)
    for nseg, L in ((2, 600), (1, 64), (1, 256), (1, 257), (0, 64), (1, 0)):
        add("mlg_op_loftr_coarse_layer_ws_bytes", nseg, L)
    for fn in ("mlg_vit_workspace_bytes", "mlg_salad_workspace_bytes"):
        for batch in (1, 64):
            for size in (28, 322, 518, 300):
                add(fn, batch, size)
        add(fn, 0, 322)
    for B in (1, 64):
        for size in (28, 322, 518, 300, 14):
            for K in (24, 64, 128, 144):
                add("mlg_anyloc_workspace_bytes", B, size, K)
    for B, P in ((1, 1), (2, 529), (64, 1369), (0, 10), (2, 0), (65536, 1)):
        for K in (16, 24, 64, 128, 144):
            add("mlg_vlad_workspace_bytes", B, P, K)
    for M, K in ((100, 8), (100, 16), (1536, 64), (1537, 64), (500000, 128), (0, 64)):
        add("mlg_kmeans_workspace_bytes", M, K)
    for N, D, Q in ((1, 1, 1), (100, 768, 100), (1000, 770, 64), (4000, 8448, 246), (0, 768, 1), (10, 0, 1)):
        add("mlg_knn_workspace_bytes", N, D, Q)
        for k in (1, 32, 33, 0):
            for query in (0, 1):
                add("mlg_knn_workspace_bytes_k", N, D, Q, k, query)
    add("mlg_knn_workspace_bytes_k", 100, 766, 100, 10, 0)  # D % 4 != 0: not fused
    add("mlg_knn_workspace_bytes_k", 100, 766, 100, 10, 1)
    for n1, n2, D in ((1, 1, 1), (528, 528, 768), (17, 33, 256), (0, 5, 4), (5, 5, 0)):
        add("mlg_xcorr_workspace_bytes", n1, n2, D)
    for F, L, D, P in ((1, 1, 4, 1), (40, 528, 768, 120), (3, 65, 768, 16384), (3, 65, 768, 16385), (2, 128, 768, 0),
                       (0, 1, 4, 1)):
        add("mlg_xcorr_batch_workspace_bytes", F, L, D, P)
    for S, it in ((1, 1), (3, 8), (64, 100), (7, 9), (0, 100), (1, 0)):
        add("mlg_plane_ransac_workspace_bytes", S, it)
    for P, S_total in ((1, 0), (1, 5), (3, 1000), (128, 100000), (0, 10), (1, -1)):
        for H in (1, 8, 1000):
            add("mlg_ransac_workspace_bytes", P, S_total, H)
    add("mlg_ransac_workspace_bytes", 1, 5, 0)
    for B, H, W in ((1, 16, 16), (1, 15, 16), (1, 16, 15), (2, 480, 640), (1, 17, 31), (0, 16, 16)):
        add("mlg_superpoint_workspace_bytes", B, H, W)
    for B, H, W in ((1, 1, 1), (1, 224, 224), (2, 480, 640), (3, 37, 1000), (0, 480, 640), (1, 0, 640)):
        add("mlg_resnet50_workspace_bytes", B, H, W)
    for B, H, W in ((1, 480, 640), (2, 480, 640), (7, 33, 17), (0, 480, 640), (1, 480, 0)):
        add("mlg_mixvpr_workspace_bytes", B, H, W)
    # ORB: params computed for a pH x pW frame, queried for F frames of H x W (the last
    # two are refused: a frame below 16 rows, and a level 0 that disagrees with the frame)
    for F, H, W, pH, pW, nf in ((1, 480, 640, 480, 640, 500), (3, 480, 640, 480, 640, 2048), (1, 64, 64, 64, 64, 100),
                                (2, 75, 131, 75, 131, 300), (0, 480, 640, 480, 640, 500), (1, 15, 640, 15, 640, 500),
                                (1, 480, 648, 480, 640, 500)):
        c.append((f"mlg_orb_workspace_bytes(params({pH}, {pW}, {nf}), {F}, {H}, {W}, {nf + 256})",
                  "mlg_orb_workspace_bytes", (("orb", pH, pW, nf), F, H, W, nf + 256)))
    for P, max_kp in ((1, 1), (1, 16), (1, 17), (3, 756), (64, 2304), (0, 756), (1, 0)):
        add("mlg_orb_match_workspace_bytes", P, max_kp)
    add("mlg_loftr_tails_bytes")
    return c


def _measure():
    from mlgate import _native
    L = _native.lib()
    L.mlg_orb_workspace_bytes.restype = ctypes.c_size_t
    L.mlg_orb_workspace_bytes.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4
    L.mlg_orb_match_workspace_bytes.restype = ctypes.c_size_t
    L.mlg_orb_match_workspace_bytes.argtypes = [ctypes.c_int] * 2
    L.mlg_loftr_features_ws_bytes.restype = ctypes.c_size_t
    L.mlg_loftr_features_ws_bytes.argtypes = [ctypes.c_int] * 3
    L.mlg_loftr_match_ws_bytes.restype = ctypes.c_size_t
    L.mlg_loftr_match_ws_bytes.argtypes = [ctypes.c_int] * 3
    out = {}
    for key, fn, args in _cases():
        keep = []  # the params buffers stay alive across the call
        cargs = []
        for a in args:
            if isinstance(a, tuple):
                keep.append(_orb_params(*a[1:]))
                cargs.append(ctypes.cast(keep[-1], ctypes.c_void_p))
            else:
                cargs.append(a)
        assert key not in out, key
        out[key] = int(getattr(L, fn)(*cargs))
    return out


@pytest.fixture(scope="module")
def measured():
    return _measure()


def test_table_covers_every_size_query():
    """Every size_t mlg_*bytes function of the public header is in the table, bar proximity
    (module docstring) and the JPEG coefficient size, which is no workspace."""
    import re
    header = open(os.path.join(ROOT, "include", "mlgate.h")).read()
    declared = set(re.findall(r"^size_t\s+(mlg_\w+)\s*\(", header, flags=re.M))
    covered = {fn for _, fn, _ in _cases()}
    assert declared - covered == {"mlg_proximity_workspace_bytes", "mlg_jpeg_coef_bytes"}


def test_workspace_sizes_match_the_recorded_table(measured):
    with open(TABLE) as f:
        want = json.load(f)
    assert set(measured) == set(want)
    diff = {k: (measured[k], want[k]) for k in want if measured[k] != want[k]}
    assert not diff, diff
    # the table holds both kinds of answer: a size, and 0 for refused arguments
    assert sum(v == 0 for v in want.values()) >= 40 and sum(v > 0 for v in want.values()) >= 150


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "multi-level-indoor-slam_amd"))
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_workspace_sizes_cpu.py --record")
    table = _measure()
    with open(TABLE, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(table)} sizes ({sum(v == 0 for v in table.values())} zero) to {TABLE}")
