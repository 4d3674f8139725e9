"""A workspace one byte short is refused with the entry point's own status (CPU only).

The entry points below compare the caller's workspace size with their carve function's
total before their first HIP call, so they can be called on a machine without a GPU: dummy
non-null pointers, well-formed struct heads, the size the matching *_workspace_bytes query
returns minus one.  Which status each returns is part of the ABI's behaviour (callers tell
"allocate more" from "bad arguments" by it where the entry point does) and differs by entry
point: MLG_EINVAL for LightGlue, SuperGlue, SuperPoint, RANSAC, proximity, the full
ResNet-50 (and its resize parity entry), AnyLoc, VLAD, k-means and the ground plane;
MLG_ENOMEM for the ViT, SALAD, kNN, xcorr, ORB, the LoFTR entry points and MixVPR.
The struct layouts mirror include/mlgate.h (a wrong size is refused at the head, with
MLG_EINVAL: the MLG_ENOMEM cases would then fail)."""
import ctypes
import struct

import pytest

from mlgate import _native

EINVAL, ENOMEM = -1, -3
P, I, F32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
HEAD = [("struct_size", ctypes.c_uint32), ("abi_version", ctypes.c_uint32)]


def _struct(name, fields, head=True):
    return type(name, (ctypes.Structure,), {"_fields_": (HEAD if head else []) + fields})


def _ptrs(prefix, n):
    return [(f"{prefix}{i}", P) for i in range(n)]


VitWeights = _struct("VitWeights", _ptrs("p", 4) + _ptrs("blk", 12 * 14) + _ptrs("n", 2) + [("packing", I)])
SaladWeights = _struct("SaladWeights", _ptrs("p", 8) + [("dust_bin", F32)])
VladVocab = _struct("VladVocab", [("centers", P), ("num_clusters", I)])
RnWeights = _struct("RnWeights", _ptrs("stem", 2) + _ptrs("blk", 16 * 8))
MixWeights = _struct("MixWeights", _ptrs("stem", 2) + _ptrs("blk", 13 * 8) + _ptrs("head", 7))
SpWeights = _struct("SpWeights", _ptrs("c", 2) + _ptrs("w", 11) + _ptrs("b", 11))
LgWeights = _struct("LgWeights", [("Wr", P)] + _ptrs("blk", 18 * 10) + _ptrs("fin", 36) + _ptrs("conf", 16) + [("ones", P)])
SgWeights = _struct("SgWeights", _ptrs("kenc", 10) + _ptrs("layer", 18 * 10) + _ptrs("fin", 2) + [("bin_score", F32)])
LoftrWeights = _struct("LoftrWeights", _ptrs("stem", 2) + _ptrs("conv", 42) + _ptrs("coarse", 64) + _ptrs("fine", 16) +
                       _ptrs("tail", 6))


class Case:
    """Dummy device pointers (never dereferenced: the size check comes first) and weights."""

    def __init__(self):
        self._buf = ctypes.create_string_buffer(1 << 16)
        self.d = P((ctypes.addressof(self._buf) + 255) & ~255)  # 256-byte aligned, non-null
        self._keep = []

    def weights(self, cls, null=(), **values):
        w = cls()
        for name, typ in cls._fields_[2:]:
            if typ is P and name not in null:
                setattr(w, name, self.d.value)
        w.struct_size, w.abi_version = ctypes.sizeof(cls), 3
        for k, v in values.items():
            setattr(w, k, v)
        self._keep.append(w)
        return ctypes.cast(ctypes.pointer(w), P)

    def host_i32(self, *vals):
        a = (ctypes.c_int32 * len(vals))(*vals)
        self._keep.append(a)
        return ctypes.cast(a, P)


def _orb_params(case, H, W, nfeatures):
    from mlgate import orb
    ip, fp = orb.geometry(H, W, nfeatures)
    body = struct.pack("<24i8f16i7f2i", *ip[:24].tolist(), *fp[:8].tolist(), *ip[24:40].tolist(), *fp[8:15].tolist(),
                       *ip[40:42].tolist())
    buf = ctypes.create_string_buffer(struct.pack("<II", 8 + len(body), 3) + body)
    case._keep.append(buf)
    return ctypes.cast(buf, P)


def _entry_points():
    """name -> (expected status, size, call(workspace_bytes))"""
    L = _native.lib()
    for fn, args in (("mlg_orb_workspace_bytes", [P] + [I] * 4), ("mlg_orb_match_workspace_bytes", [I] * 2),
                     ("mlg_loftr_features_ws_bytes", [I] * 3), ("mlg_loftr_match_ws_bytes", [I] * 3)):
        getattr(L, fn).restype, getattr(L, fn).argtypes = ctypes.c_size_t, args
    L.mlg_orb_detect.restype = L.mlg_orb_match.restype = L.mlg_loftr_features.restype = L.mlg_loftr_match.restype = I
    L.mlg_superglue.restype = I
    c = Case()
    d, z, lng = c.d, ctypes.c_size_t, ctypes.c_long
    fs = lng(480 * 640 * 3)
    E = {}
    vit = c.weights(VitWeights, packing=0)
    E["mlg_vit_forward"] = (ENOMEM, L.mlg_vit_workspace_bytes(2, 322),
                            lambda n: L.mlg_vit_forward(vit, d, 2, 480, 640, 3, fs, 322, 0, d, n, d, None, None))
    salad = c.weights(SaladWeights)
    E["mlg_salad_forward"] = (ENOMEM, L.mlg_salad_workspace_bytes(2, 322),
                              lambda n: L.mlg_salad_forward(vit, salad, d, 2, 480, 640, 3, fs, 322, d, n, d, None))
    vocab = c.weights(VladVocab, num_clusters=64)
    E["mlg_anyloc_forward"] = (EINVAL, L.mlg_anyloc_workspace_bytes(1, 518, 64),
                               lambda n: L.mlg_anyloc_forward(vit, vocab, d, 1, 480, 640, 3, fs, 518, 0, d, n, d, None))
    E["mlg_op_vlad"] = (EINVAL, L.mlg_vlad_workspace_bytes(2, 529, 64),
                        lambda n: L.mlg_op_vlad(vocab, d, 2, 529, d, n, d, None, None))
    E["mlg_kmeans_step"] = (EINVAL, L.mlg_kmeans_workspace_bytes(5000, 64),
                            lambda n: L.mlg_kmeans_step(d, 5000, d, 64, d, d, d, d, n, None))
    for k, tag in ((20, "fused"), (33, "matrix")):
        E[f"mlg_knn_gate[{tag}]"] = (ENOMEM, L.mlg_knn_workspace_bytes_k(100, 768, 100, k, 0),
                                     lambda n, k=k: L.mlg_knn_gate(d, 100, 768, d, d, d, 10.0, 0.5, k, 1, 0, 100, d, n, d,
                                                                   d, d, d, None, None))
        E[f"mlg_knn_query[{tag}]"] = (ENOMEM, L.mlg_knn_workspace_bytes_k(100, 768, 7, k, 1),
                                      lambda n, k=k: L.mlg_knn_query(d, 100, 768, d, 7, d, d, 10.0, k, d, n, d, d, d,
                                                                     None))
    E["mlg_xcorr_score"] = (ENOMEM, L.mlg_xcorr_workspace_bytes(17, 33, 256),
                            lambda n: L.mlg_xcorr_score(d, 17, d, 33, 256, d, n, d, None))
    E["mlg_xcorr_batch"] = (ENOMEM, L.mlg_xcorr_batch_workspace_bytes(3, 65, 768, 5),
                            lambda n: L.mlg_xcorr_batch(d, 3, 65, 768, d, d, 5, d, n, d, None))
    E["mlg_plane_ransac"] = (EINVAL, L.mlg_plane_ransac_workspace_bytes(3, 100),
                             lambda n: L.mlg_plane_ransac(d, d, 3, 100, 0, 0.1, d, n, d, d, d, None))
    E["mlg_proximity_count"] = (EINVAL, L.mlg_proximity_workspace_bytes(5000, 100),
                                lambda n: L.mlg_proximity_count(d, None, 5000, 0, 100, 1.0, 10, 1, d, n, d, None))
    E["mlg_proximity_emit"] = (EINVAL, L.mlg_proximity_workspace_bytes(5000, 100),
                               lambda n: L.mlg_proximity_emit(d, None, 5000, 0, 100, 1.0, 10, 1, d, n, d, d, d, None))
    E["mlg_ransac_epipolar"] = (EINVAL, L.mlg_ransac_workspace_bytes(3, 1000, 8),
                                lambda n: L.mlg_ransac_epipolar(d, d, d, 3, 1000, d, 0, 3.0, 8, 0, d, n, d, d, d, None, d,
                                                                None))
    first = {0, 3, 7, 13}  # the blocks that carry a downsample conv
    rn = c.weights(RnWeights, null={f"blk{8 * i + j}" for i in range(16) if i not in first for j in (6, 7)})
    E["mlg_resnet50_forward"] = (EINVAL, L.mlg_resnet50_workspace_bytes(2, 480, 640),
                                 lambda n: L.mlg_resnet50_forward(rn, d, 2, 480, 640, 3, fs, 4096, d, n, d, None))
    E["mlg_op_pillow_resize_224"] = (EINVAL, L.mlg_resnet50_workspace_bytes(2, 480, 640),
                                     lambda n: L.mlg_op_pillow_resize_224(d, 2, 480, 640, 3, fs, d, n, d, None))
    mix = c.weights(MixWeights, null={f"blk{8 * i + j}" for i in range(13) if i not in first for j in (6, 7)})
    E["mlg_mixvpr_forward"] = (ENOMEM, L.mlg_mixvpr_workspace_bytes(2, 480, 640),
                               lambda n: L.mlg_mixvpr_forward(mix, d, 2, 480, 640, 3, fs, d, n, d, None))
    sp = c.weights(SpWeights)
    E["mlg_superpoint"] = (EINVAL, L.mlg_superpoint_workspace_bytes(1, 480, 640),
                           lambda n: L.mlg_superpoint(sp, d, 1, 480, 640, 3, fs, 0.0005, 2048, 4, 4, d, n, d, d, d, None,
                                                      d, None))
    pa, pb, counts = c.host_i32(0, 1), c.host_i32(1, 2), c.host_i32(65, 64, 1)
    lg = c.weights(LgWeights)
    E["mlg_lightglue"] = (EINVAL, L.mlg_lightglue_workspace_bytes(2, 65),
                          lambda n: L.mlg_lightglue(lg, d, d, counts, 3, 65, pa, pb, 2, 0.95, 0.99, 0.1, 1536, d, n, d, d,
                                                    d, None, None))
    sg = c.weights(SgWeights)
    L.mlg_superglue.argtypes = [P] * 5 + [I] * 4 + [P, P, I, I, F32, P, z, P, P, P, P]
    E["mlg_superglue"] = (EINVAL, L.mlg_superglue_workspace_bytes(2, 65),
                          lambda n: L.mlg_superglue(sg, d, d, d, counts, 3, 65, 640, 480, pa, pb, 2, 20, 0.2, d, n, d, d,
                                                    d, None))
    lf = c.weights(LoftrWeights)
    L.mlg_loftr_features.argtypes = [P, P, I, I, I, I, lng, P, z, P, P, P]
    L.mlg_loftr_match.argtypes = [P, P, P, I, I, P, P, I, P, P, z, P, P, P, P, P]
    for H, W in ((480, 640), (100, 99)):
        E[f"mlg_loftr_features[{H}x{W}]"] = (ENOMEM, L.mlg_loftr_features_ws_bytes(1, H, W),
                                             lambda n, H=H, W=W: L.mlg_loftr_features(lf, d, 1, H, W, 3, lng(H * W * 3), d,
                                                                                      n, d, d, None))
    for Pn in (1, 9):  # 32 x 32, one pair: csplit in its own region
        E[f"mlg_loftr_match[{Pn}]"] = (ENOMEM, L.mlg_loftr_match_ws_bytes(Pn, 32, 32),
                                       lambda n, Pn=Pn: L.mlg_loftr_match(lf, d, d, 32, 32, d, d, Pn, d, d, n, d, d, d, d,
                                                                          None))
    E["mlg_op_loftr_coarse_layer"] = (ENOMEM, L.mlg_op_loftr_coarse_layer_ws_bytes(2, 600),
                                      lambda n: L.mlg_op_loftr_coarse_layer(lf, 1, 1, d, d, 2, 600, d, n, None))
    orbp = _orb_params(c, 480, 640, 500)
    L.mlg_orb_detect.argtypes = [P, P, P, lng, I, I, I, I, I, P, z] + [P] * 7
    L.mlg_orb_match.argtypes = [P, P, I, P, P, I, P, z, P, P, P, P, P]
    E["mlg_orb_detect"] = (ENOMEM, L.mlg_orb_workspace_bytes(orbp, 2, 480, 640, 756),
                           lambda n: L.mlg_orb_detect(orbp, d, d, fs, 2, 480, 640, 3, 756, d, n, d, d, d, d, d, d, None))
    E["mlg_orb_match"] = (ENOMEM, L.mlg_orb_match_workspace_bytes(3, 756),
                          lambda n: L.mlg_orb_match(d, d, 756, d, d, 3, d, n, d, d, d, d, None))
    return c, E


@pytest.fixture(scope="module")
def entry_points():
    return _entry_points()


NAMES = ["mlg_vit_forward", "mlg_salad_forward", "mlg_anyloc_forward", "mlg_op_vlad", "mlg_kmeans_step",
         "mlg_knn_gate[fused]", "mlg_knn_gate[matrix]", "mlg_knn_query[fused]", "mlg_knn_query[matrix]", "mlg_xcorr_score",
         "mlg_xcorr_batch", "mlg_plane_ransac", "mlg_proximity_count", "mlg_proximity_emit", "mlg_ransac_epipolar",
         "mlg_resnet50_forward", "mlg_op_pillow_resize_224", "mlg_mixvpr_forward", "mlg_superpoint", "mlg_lightglue",
         "mlg_superglue", "mlg_loftr_features[480x640]", "mlg_loftr_features[100x99]", "mlg_loftr_match[1]",
         "mlg_loftr_match[9]", "mlg_op_loftr_coarse_layer", "mlg_orb_detect", "mlg_orb_match"]


def test_every_case_is_listed(entry_points):
    assert sorted(entry_points[1]) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_short_workspace_status(entry_points, name):
    want, size, call = entry_points[1][name]
    assert size > 0, "the size query refused the arguments"
    assert call(ctypes.c_size_t(size - 1)) == want
    assert call(ctypes.c_size_t(0)) == want
