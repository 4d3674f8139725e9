"""numpy restatement of the device half of JPEG ingestion (csrc/jpeg.hip): quantised DCT
coefficients -> BGR pixels with libjpeg's integer arithmetic -- dequantise,
jpeg_idct_islow, fancy h2v1 / h2v2 chroma upsampling (replication when the downsampled
width is <= 2), the 16-bit fixed-point YCbCr conversion.  A test helper: the CPU tests
run the host decoder's output through it and compare with libjpeg-turbo's own pixels.

All arithmetic is int32 and wraps, as the kernel's does; ``>>`` is arithmetic.
"""
import numpy as np

PARAMS = 16  # MLG_JPEG_PARAMS
EINVAL, ESIZE, EUNSUP = -1, -4, -5

_cases = None


def load_cases():
    """tests/golden/jpeg_cases.npz (tests/golden/make_jpeg_goldens.py) as a list of dicts
    name / kind / blob (bytes) / bgr (uint8 [H, W, 3] or None), plus the sequence's
    timestamps and floors.  Loaded once and shared: treat as read-only."""
    global _cases
    if _cases is None:
        import lzma
        import os
        d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz"))
        blobs, px = lzma.decompress(d["blob_xz"].tobytes()), lzma.decompress(d["bgr_xz"].tobytes())
        cases, bo, po = [], 0, 0
        for name, kind, n, (h, w) in zip(d["names"], d["kinds"], d["blob_len"], d["bgr_shape"]):
            bgr = None
            if h:
                planar = np.frombuffer(px, np.uint8, 3 * h * w, po).reshape(3, h, w)
                bgr = np.ascontiguousarray(np.cumsum(planar, axis=2, dtype=np.uint8).transpose(1, 2, 0))
                bgr.setflags(write=False)
                po += 3 * h * w
            cases.append({"name": str(name), "kind": str(kind), "blob": blobs[bo:bo + int(n)], "bgr": bgr})
            bo += int(n)
        _cases = (cases, d["seq_t"], d["seq_floor"])
    return _cases


def _descale(x, n):
    return (x + np.int32(1 << (n - 1))) >> n


def _islow_1d(v, shift):
    """One pass of jpeg_idct_islow over the first axis of v (int32 [8, ...])."""
    c = np.int32
    z2, z3 = v[2], v[6]
    z1 = (z2 + z3) * c(4433)
    tmp2 = z1 + z3 * c(-15137)
    tmp3 = z1 + z2 * c(6270)
    z2, z3 = v[0], v[4]
    tmp0 = (z2 + z3) << 13
    tmp1 = (z2 - z3) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * c(9633)
    tmp0, tmp1, tmp2, tmp3 = tmp0 * c(2446), tmp1 * c(16819), tmp2 * c(25172), tmp3 * c(12299)
    z1, z2 = z1 * c(-7373), z2 * c(-20995)
    z3, z4 = z3 * c(-16069) + z5, z4 * c(-3196) + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return np.stack([_descale(tmp10 + tmp3, shift), _descale(tmp11 + tmp2, shift), _descale(tmp12 + tmp1, shift),
                     _descale(tmp13 + tmp0, shift), _descale(tmp13 - tmp0, shift), _descale(tmp12 - tmp1, shift),
                     _descale(tmp11 - tmp2, shift), _descale(tmp10 - tmp3, shift)])


def idct_plane(blocks, q):
    """int16 [brows, bcols, 64] coefficients, uint16 [64] table -> uint8 [brows*8, bcols*8]."""
    brows, bcols, _ = blocks.shape
    with np.errstate(over="ignore"):
        d = blocks.astype(np.int32) * q.astype(np.int32)
        d = d.reshape(brows, bcols, 8, 8)                      # [.., row, col]
        cols = _islow_1d(np.moveaxis(d, 2, 0), 11)             # down each column: axis 0 = row index
        rows = _islow_1d(np.moveaxis(cols, 3, 0), 18)          # along each row: [col, row, brows, bcols]
    px = np.clip(rows + 128, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(px.transpose(2, 1, 3, 0)).reshape(brows * 8, bcols * 8)


def _h2v1_fancy(p):
    """[h, cw] -> [h, 2*cw]"""
    a = p.astype(np.int32)
    out = np.empty((a.shape[0], 2 * a.shape[1]), np.int32)
    left = np.concatenate([a[:, :1], a[:, :-1]], 1)
    right = np.concatenate([a[:, 1:], a[:, -1:]], 1)
    out[:, 0::2] = (3 * a + left + 1) >> 2
    out[:, 1::2] = (3 * a + right + 2) >> 2
    out[:, 0] = a[:, 0]
    out[:, -1] = a[:, -1]
    return out


def _h2v2_fancy(p):
    """[ch, cw] -> [2*ch, 2*cw]"""
    a = p.astype(np.int32)
    up = np.concatenate([a[:1], a[:-1]], 0)
    down = np.concatenate([a[1:], a[-1:]], 0)
    out = np.empty((2 * a.shape[0], 2 * a.shape[1]), np.int32)
    for par, near in ((0, up), (1, down)):
        s = 3 * a + near
        left = np.concatenate([s[:, :1], s[:, :-1]], 1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
        o = np.empty((a.shape[0], 2 * a.shape[1]), np.int32)
        o[:, 0::2] = (3 * s + left + 8) >> 4
        o[:, 1::2] = (3 * s + right + 7) >> 4
        o[:, 0] = (4 * s[:, 0] + 8) >> 4
        o[:, -1] = (4 * s[:, -1] + 7) >> 4
        out[par::2] = o
    return out


def pixels(coefs, qtabs, params, H, W):
    """One image: int16 coefficient buffer, uint16 [3, 64] tables, int32 [16] record ->
    uint8 [H, W, 3] BGR."""
    coefs = np.asarray(coefs).reshape(-1)
    qtabs = np.asarray(qtabs).reshape(3, 64)
    p = [int(x) for x in np.asarray(params).reshape(-1)[:PARAMS]]
    nc, hmax, vmax = p[0], p[1], p[2]
    planes = []
    for c in range(nc):
        bcols, brows, off = p[4 + 4 * c], p[5 + 4 * c], p[6 + 4 * c]
        blocks = coefs[off:off + brows * bcols * 64].reshape(brows, bcols, 64)
        full = idct_plane(blocks, qtabs[c])
        sx, sy = (1, 1) if c == 0 else (hmax, vmax)
        cw, ch = -(-W // sx), -(-H // sy)
        pl = full[:ch, :cw]
        if sx == 2:
            if cw <= 2:
                pl = np.repeat(np.repeat(pl, sy, 0), 2, 1)
            elif sy == 1:
                pl = _h2v1_fancy(pl)
            else:
                pl = _h2v2_fancy(pl)
        planes.append(pl[:H, :W].astype(np.int32))
    y = planes[0]
    if nc == 1:
        g = y.astype(np.uint8)
        return np.stack([g, g, g], -1)
    cb, cr = planes[1] - 128, planes[2] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)
