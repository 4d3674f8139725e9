"""Keyframe ingestion: PNG and JPEG keyframe files -> BGR uint8
frames in HBM.

Replaces the per-image ``cv2.imread(str(path))`` loop of ``process_image_sequence``
(place_recognition.py:936-991) for the '{timestamp:.6f}.png' keyframes that
``extract_images`` (scripts/utils/bag_utils.py:222-271) writes and for the ``*.jpg``
files the reference reads after them.  PNG decoding is host work (DEFLATE and the PNG
row filters are serial per image): ``mlg_png_load_bgr`` decodes a batch on a pool of
host threads straight into a page-locked buffer.  A JPEG is split: the same kind of pool
Huffman-decodes a batch to quantised DCT coefficients (``mlg_jpeg_coefs_load``), and the
inverse DCT, chroma upsampling and colour conversion run on the GPU
(``torch.ops.mlgate.jpeg_pixels``), with libjpeg-turbo's integers.  ``KeyframeStream``
copies each batch to HBM on a side stream while the caller's stream runs the previous
batch through the ViT (two pinned buffers, an event per buffer).
"""
import os
import struct
import warnings
import zlib
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import _native

DEFAULT_THREADS = min(16, os.cpu_count() or 1)
_SIG = b"\x89PNG\r\n\x1a\n"


def png_info(data: bytes) -> Optional[Tuple[int, int, int, int]]:
    """(width, height, color_type, bit_depth) from a PNG's IHDR (CRC-checked), None if
    the bytes do not start like a PNG."""
    if len(data) < 33 or data[:8] != _SIG or data[12:16] != b"IHDR" or struct.unpack(">I", data[8:12])[0] != 13:
        return None
    if zlib.crc32(data[12:29]) & 0xFFFFFFFF != struct.unpack(">I", data[29:33])[0]:
        return None
    w, h, depth, ctype = struct.unpack(">IIBB", data[16:26])
    return (w, h, ctype, depth) if w and h else None


def _header(path) -> Optional[Tuple[int, int]]:
    try:
        with open(path, "rb") as f:
            info = png_info(f.read(33))
    except OSError:
        return None
    return None if info is None else (info[1], info[0])


def decode_png_bytes(blobs: Sequence[bytes], H: int, W: int,
                     threads: int = DEFAULT_THREADS) -> Tuple[np.ndarray, np.ndarray]:
    """Decode in-memory PNGs of one size -> (uint8 [n, H, W, 3] BGR, int32 status [n])."""
    import torch
    ts = [torch.frombuffer(bytearray(b), dtype=torch.uint8) if len(b) else torch.zeros(0, dtype=torch.uint8)
          for b in blobs]
    out, status = _native.ops().png_decode(ts, int(H), int(W), int(threads))
    return out.numpy(), status.numpy()


def load_png_batch(paths: Sequence, H: int, W: int, out, threads: int = DEFAULT_THREADS) -> np.ndarray:
    """Decode PNG files of size H x W into the host uint8 tensor ``out`` (>= n*H*W*3
    bytes; page-locked for an async upload); returns the per-file status (0 ok)."""
    return _native.ops().png_load_into([os.fspath(p) for p in paths], out, int(H), int(W), int(threads)).numpy()


def imread(path) -> Optional[np.ndarray]:
    """``cv2.imread(path)`` (IMREAD_COLOR) for a PNG file: BGR uint8 [H, W, 3] or None."""
    import torch
    hw = _header(path)
    if hw is None:
        return None
    out = torch.empty((1, hw[0], hw[1], 3), dtype=torch.uint8)
    st = load_png_batch([path], hw[0], hw[1], out, threads=1)
    return out[0].numpy() if st[0] == 0 else None


def jpeg_info(data: bytes) -> Optional[Tuple[int, int, int, int, int, bool]]:
    """(width, height, components, luma_h, luma_v, supported) from a JPEG's headers (read
    up to SOS), None if the bytes are not a JPEG header.  ``supported`` says whether the
    native path decodes the stream; every other file stays with ``jpeg_reader()``."""
    import torch
    if len(data) < 4:
        return None
    r = _native.ops().jpeg_info(torch.frombuffer(bytearray(data), dtype=torch.uint8)).tolist()
    return None if r[0] != 0 else (r[1], r[2], r[3], r[4], r[5], bool(r[6]))


_JPEG_HEAD = 1 << 16


def _jpeg_header(path) -> Optional[Tuple[int, int]]:
    """(H, W) of a JPEG file the native path accepts, else None."""
    try:
        with open(path, "rb") as f:
            data = f.read(_JPEG_HEAD)
            info = jpeg_info(data)
            if info is None and len(data) == _JPEG_HEAD:  # headers longer than the first read (Exif, ICC)
                info = jpeg_info(data + f.read())
    except OSError:
        return None
    return (info[1], info[0]) if info is not None and info[5] else None


class _JpegStage:
    """Views of one host byte buffer as the three outputs of the coefficient decoder for
    n images of H x W: [coefs | qtabs | params]; coefs + qtabs are uploaded as one block."""

    def __init__(self, buf, n: int, H: int, W: int):
        import torch
        per = int(_native.ops().jpeg_coef_bytes(int(H), int(W)))
        self.n, self.H, self.W, self.per = n, H, W, per
        self.upload = n * (per + 384)
        self.bytes = self.upload + n * 64
        b = buf[:self.bytes]
        self.coefs = b[:n * per].view(torch.int16)
        self.qtabs = b[n * per:self.upload].view(torch.uint16)
        self.params = b[self.upload:].view(torch.int32)

    @staticmethod
    def nbytes(n: int, H: int, W: int) -> int:
        return n * (int(_native.ops().jpeg_coef_bytes(int(H), int(W))) + 384 + 64)

    def pixels(self, dev_buf):
        """jpeg_pixels over the uploaded copy `dev_buf` of the first `upload` bytes."""
        import torch
        n, per = self.n, self.per
        return _native.ops().jpeg_pixels(dev_buf[:n * per].view(torch.int16),
                                         dev_buf[n * per:self.upload].view(torch.uint16),
                                         self.params.clone().view(n, 16), int(self.H), int(self.W))


def decode_jpeg_bytes(blobs: Sequence[bytes], H: int, W: int, device="cuda",
                      threads: int = DEFAULT_THREADS):
    """Decode in-memory JPEGs of one size -> (uint8 [n, H, W, 3] BGR tensor on `device`,
    int32 status [n] numpy).  Huffman decode on host threads, IDCT / upsampling / colour on
    the GPU.  The frame of an image whose status is not 0 is zero."""
    import torch
    dev = _native.require_device(device)
    n = len(blobs)
    ts = [torch.frombuffer(bytearray(b), dtype=torch.uint8) if len(b) else torch.zeros(0, dtype=torch.uint8)
          for b in blobs]
    host = torch.empty(max(1, _JpegStage.nbytes(n, H, W)), dtype=torch.uint8)
    st = _JpegStage(host, n, H, W)
    status = _native.ops().jpeg_coefs_decode(ts, st.coefs, st.qtabs, st.params, int(H), int(W), int(threads)).numpy()
    if n == 0:
        return torch.empty((0, H, W, 3), dtype=torch.uint8, device=dev), status
    with torch.cuda.device(dev):
        frames = st.pixels(host[:st.upload].to(dev))
    bad = np.nonzero(status)[0]
    if len(bad):
        frames[torch.from_numpy(bad).to(dev)] = 0
    return frames, status


def load_jpeg_coefs(paths: Sequence, H: int, W: int, stage: "_JpegStage", threads: int = DEFAULT_THREADS) -> np.ndarray:
    """Huffman-decode JPEG files of size H x W into the host stage; per-file status (0 ok)."""
    return _native.ops().jpeg_coefs_load_into([os.fspath(p) for p in paths], stage.coefs, stage.qtabs, stage.params,
                                              int(H), int(W), int(threads)).numpy()


def jpeg_reader():
    """A ``path -> BGR uint8 [H, W, 3] or None`` JPEG reader: cv2.imread when OpenCV is
    installed (the reference's call), else Pillow (the same libjpeg-turbo decoder with
    OpenCV's defaults: islow IDCT, fancy upsampling), converted to RGB and channel-swapped.
    Raises the reference's ImportError when neither is available."""
    try:
        import cv2
        return lambda p: cv2.imread(str(p))
    except ImportError:
        pass
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("OpenCV is required for image loading. Install with: pip install opencv-python") from e

    def read(p):
        try:
            with Image.open(p) as im:
                return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])
        except (OSError, ValueError):
            return None
    return read


_JPEG_EXT = (".jpg", ".jpeg")


class KeyframeStream:
    """Iterate over PNG and JPEG keyframes in device batches: yields ``(indices, frames)``
    with ``frames`` a uint8 [b, H, W, 3] BGR tensor on ``device`` and ``indices`` the
    positions in ``paths`` it holds, in the order of ``paths``.  Consecutive files of one
    kind and frame size form a batch; a file of another size is decoded in a batch of its
    own size.  Decode of batch i + 1 overlaps the caller's work on batch i; the upload runs
    on a side stream and the consumer's stream waits for it by event.

    PNG: files that fail to decode are skipped with the reference's warning ("Failed to
    load image: ...").  JPEG (``.jpg`` / ``.jpeg``): the native path uploads coefficients and
    ``jpeg_pixels`` produces the frames on the consumer's stream; a file it declines
    (progressive, CMYK, an Exif rotation, a damaged stream, ...) is read by ``jpeg_reader()``
    -- what every JPEG went through before -- and joins the stream at its own position;
    only when that reader returns None too is the warning given.  ``jpeg_reader()`` is
    looked up on first need, so its ImportError appears only if a fallback is needed.
    """

    def __init__(self, paths: Sequence, device="cuda", batch: int = 123, threads: int = DEFAULT_THREADS):
        import torch
        _native.require_device(device)
        self.paths = [str(p) for p in paths]
        self.device = torch.device(device)
        self.batch = int(batch)
        self.threads = int(threads)
        self._torch = torch
        self._reader = None

    def _groups(self) -> List[Tuple[str, Optional[Tuple[int, int]], List[int]]]:
        """Consecutive runs of one kind ('png', 'jpeg', or 'legacy': a JPEG for
        jpeg_reader()) and frame size, in file order, at most `batch` long."""
        groups, cur, key = [], [], None
        for i, p in enumerate(self.paths):
            if p.lower().endswith(_JPEG_EXT):
                hw = _jpeg_header(p)
                k = ("jpeg", hw) if hw is not None else ("legacy", None)
            else:
                hw = _header(p)
                if hw is None:
                    warnings.warn(f"Failed to load image: {p}")
                    continue
                k = ("png", hw)
            if cur and (k != key or k[0] == "legacy" or len(cur) == self.batch):
                groups.append((key[0], key[1], cur))
                cur = []
            key = k
            cur.append(i)
        if cur:
            groups.append((key[0], key[1], cur))
        return groups

    def _legacy(self, path):
        """BGR uint8 [H, W, 3] host array from jpeg_reader(), or None after the warning."""
        if self._reader is None:
            self._reader = jpeg_reader()
        img = self._reader(path)
        if img is None or getattr(img, "ndim", 0) != 3 or img.shape[2] != 3:
            warnings.warn(f"Failed to load image: {path}")
            return None
        return np.ascontiguousarray(img, dtype=np.uint8)

    def __iter__(self) -> Iterator[Tuple[List[int], "object"]]:
        torch = self._torch
        side = torch.cuda.Stream(device=self.device)
        consumer = torch.cuda.current_stream(self.device)
        pinned = [None, None]
        done = [None, None]
        slot = 1
        for kind, hw, idx in self._groups():
            if kind == "legacy":
                img = self._legacy(self.paths[idx[0]])
                if img is not None:
                    yield idx, torch.from_numpy(img).to(self.device)[None]
                continue
            H, W = hw
            n = len(idx)
            slot ^= 1
            need = n * H * W * 3 if kind == "png" else _JpegStage.nbytes(n, H, W)
            if done[slot] is not None:
                done[slot].synchronize()  # the upload that last read this pinned buffer finished
            if pinned[slot] is None or pinned[slot].numel() < need:
                pinned[slot] = torch.empty(need, dtype=torch.uint8, pin_memory=True)
            host = pinned[slot]
            names = [self.paths[i] for i in idx]
            if kind == "png":
                status = load_png_batch(names, H, W, host, self.threads)
                nup = need
            else:
                stage = _JpegStage(host, n, H, W)
                status = load_jpeg_coefs(names, H, W, stage, self.threads)
                nup = stage.upload
            ok = [k for k, s in enumerate(status) if s == 0]
            # what replaces a failed file: nothing for a PNG; for a JPEG the legacy reader's pixels
            late = {}
            for k, s in enumerate(status):
                if s == 0:
                    continue
                if kind == "png":
                    warnings.warn(f"Failed to load image: {names[k]}")
                else:
                    img = self._legacy(names[k])
                    if img is not None:
                        late[k] = img
            if not ok and not late:
                continue
            frames = None
            if ok:
                with torch.cuda.device(self.device):
                    dev = torch.empty(nup, dtype=torch.uint8, device=self.device)
                    side.wait_stream(consumer)  # `dev` may reuse memory the consumer still reads
                    with torch.cuda.stream(side):
                        dev.copy_(host[:nup], non_blocking=True)
                        ev = torch.cuda.Event()
                        ev.record(side)
                    done[slot] = ev
                    consumer.wait_event(ev)
                    dev.record_stream(consumer)
                    frames = dev.view(n, H, W, 3) if kind == "png" else stage.pixels(dev)
            # runs of positions that share the batch's frame size go out as one tensor
            keep = sorted(set(ok) | set(late))
            run = []
            for k in keep + [None]:
                fits = k is not None and (k not in late or late[k].shape[:2] == (H, W))
                if fits:
                    run.append(k)
                    continue
                if run:
                    yield [idx[r] for r in run], self._gather(frames, run, late, (H, W))
                    run = []
                if k is not None:
                    yield [idx[k]], torch.from_numpy(late[k]).to(self.device)[None]
        for ev in done:
            if ev is not None:
                ev.synchronize()

    def _gather(self, frames, run, late, hw):
        """The frames of positions `run` of a batch: natively decoded ones from `frames`,
        the others from the legacy reader's arrays."""
        torch = self._torch
        if frames is None:
            return torch.from_numpy(np.stack([late[k] for k in run])).to(self.device)
        for k in run:
            if k in late:
                frames[k] = torch.from_numpy(late[k]).to(self.device)
        if len(run) == frames.shape[0]:
            return frames
        return frames[torch.tensor(run, device=self.device)]
