"""CricaVPR's head restated in numpy (tests/test_crica_cpu.py, tests/test_crica_gpu.py).

Upstream CricaVPRNet.forward (Lu-Feng/CricaVPR) over the final-LayerNormed tokens of DINOv2
ViT-B/14, written from its description (include/mlgate.h "CricaVPR"), independent of
csrc/crica.hip and of torch.nn:

  pool        LayerNorm (eps 1e-6) of [1 + g^2, 768] tokens, then ``pyramid``
  pyramid     14 rows: the CLS token; the patch tokens L2-normalised per token, then GeM
              (mean(clamp(x, 1e-6)^p)^(1/p)) over upstream's literal slices: [0:8], [8:g] both
              ways (rows 1-4), [0:5], [5:11], [11:g] both ways (rows 5-13), row band major
  encode      2 post-LN transformer encoder layers (16 heads of 48, feed-forward 2048, erf
              GELU, LayerNorm eps 1e-5) whose sequence axis is the images of a group, then the
              14 x 768 values of a frame divided by max(|.|, 1e-12)
  descriptor  encode(pool(...))

Each takes ``mode``: "f64" (the reference), "f32" (every array and operation float32: the
rounding floor e_f32 of a float32 implementation) and, for ``encode``, "split" (float64, but
every GEMM operand rounded to a bf16 hi + lo pair and the lo * lo product dropped: a model of
the split-bf16 arithmetic, printed beside the measured error, never used as a bar).
"""
import functools
import math

import numpy as np
import torch

from mlgate import weights as W

E, ROWS, HEADS, HD, FF, LAYERS = 768, 14, 16, 48, 2048, 2
DIM = ROWS * E
L1_CUTS, L2_CUTS = (0, 8, None), (0, 5, 11, None)


def regions(g):
    """The 13 (row slice, column slice) pairs in output order (rows 1..13 of the pyramid)."""
    out = []
    for cuts in (L1_CUTS, L2_CUTS):
        bands = [slice(a, g if b is None else b) for a, b in zip(cuts[:-1], cuts[1:])]
        out += [(r, c) for r in bands for c in bands]
    return out


def _dt(mode):
    return np.float32 if mode == "f32" else np.float64


def layernorm(x, w, b, eps, mode="f64"):
    dt = _dt(mode)
    x, w, b = x.astype(dt), np.asarray(w, dt), np.asarray(b, dt)
    mean = x.mean(axis=-1, keepdims=True, dtype=dt)
    var = np.mean((x - mean) ** 2, axis=-1, keepdims=True, dtype=dt)
    return ((x - mean) / np.sqrt(var + dt(eps)) * w + b).astype(dt)


def pyramid(normed, p, mode="f64"):
    """normed: [B, 1 + g^2, 768] final-normed tokens, CLS first -> [B, 14, 768]."""
    dt = _dt(mode)
    x = normed.astype(dt)
    B, T, _ = x.shape
    g = math.isqrt(T - 1)
    assert g * g + 1 == T
    patches = x[:, 1:]
    nrm = np.sqrt(np.sum(patches * patches, axis=-1, keepdims=True, dtype=dt))
    unit = (patches / np.maximum(nrm, dt(1e-12))).reshape(B, g, g, E)
    powed = np.power(np.maximum(unit, dt(1e-6)), dt(p))
    rows = [x[:, 0]]
    for rs, cs in regions(g):
        m = powed[:, rs, cs].reshape(B, -1, E).mean(axis=1, dtype=dt)
        rows.append(np.power(m, dt(1.0) / dt(p)))
    return np.stack(rows, axis=1).astype(dt)


def pool(tokens_prenorm, norm_w, norm_b, p, mode="f64"):
    return pyramid(layernorm(tokens_prenorm, norm_w, norm_b, 1e-6, mode), p, mode)


def _bf16_pair(a):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    hi = t.bfloat16().float()
    lo = (t - hi).bfloat16().float()
    return hi.double().numpy(), lo.double().numpy()


def _linear(x, w, b, mode):
    if mode == "split":  # the operands as the f32 values the kernels hold, split in two
        xh, xl = _bf16_pair(x)
        wh, wl = _bf16_pair(w)
        return xh @ wh.T + xh @ wl.T + xl @ wh.T + np.asarray(b, np.float64)
    dt = _dt(mode)
    return (x.astype(dt) @ np.asarray(w, dt).T + np.asarray(b, dt)).astype(dt)


def _gelu(x):
    return (x * 0.5 * (1.0 + torch.erf(torch.from_numpy(x / np.sqrt(x.dtype.type(2.0)))).numpy())).astype(x.dtype)


def _layer(x, sd, i, mode):
    """x: [n, 14, 768], the n images of one group."""
    dt = _dt(mode)
    k = lambda s: sd[f"encoder.layers.{i}.{s}"]  # noqa: E731
    n = x.shape[0]
    qkv = _linear(x.reshape(n * ROWS, E), k("self_attn.in_proj_weight"), k("self_attn.in_proj_bias"), mode)
    q, kk, v = (qkv[:, j * E:(j + 1) * E].reshape(n, ROWS, HEADS, HD) for j in range(3))
    s = np.einsum("irhd,jrhd->rhij", q * dt(HD ** -0.5), kk).astype(dt)
    s = np.exp(s - s.max(axis=-1, keepdims=True))
    a = (s / s.sum(axis=-1, keepdims=True, dtype=dt)).astype(dt)
    o = np.einsum("rhij,jrhd->irhd", a, v).astype(dt).reshape(n * ROWS, E)
    y = _linear(o, k("self_attn.out_proj.weight"), k("self_attn.out_proj.bias"), mode)
    x1 = layernorm(x.reshape(n * ROWS, E).astype(dt) + y, k("norm1.weight"), k("norm1.bias"), 1e-5, mode)
    h = _gelu(_linear(x1, k("linear1.weight"), k("linear1.bias"), mode))
    y = _linear(h, k("linear2.weight"), k("linear2.bias"), mode)
    return layernorm(x1 + y, k("norm2.weight"), k("norm2.bias"), 1e-5, mode).reshape(n, ROWS, E)


def groups(B, group):
    return [(f, min(B, f + group)) for f in range(0, B, group)]


def encode(pooled, sd, group=1, mode="f64"):
    """pooled: [B, 14, 768] -> unit descriptors [B, 10752]."""
    dt = _dt(mode)
    x = pooled.astype(dt)
    out = np.empty((x.shape[0], DIM), dt)
    for f0, f1 in groups(x.shape[0], group):
        y = x[f0:f1]
        for i in range(LAYERS):
            y = _layer(y, sd, i, mode)
        flat = y.reshape(f1 - f0, DIM)
        nrm = np.sqrt(np.sum(flat * flat, axis=1, keepdims=True, dtype=dt))
        out[f0:f1] = flat / np.maximum(nrm, dt(1e-12))
    return out


def descriptor(normed, sd, group=1, mode="f64"):
    """Final-normed tokens [B, 1 + g^2, 768] (CLS first) -> unit descriptors [B, 10752]."""
    p = float(np.asarray(sd["aggregation.1.p"]).reshape(-1)[0])
    return encode(pyramid(normed, p, mode), sd, group, mode)


def one_minus_cos(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(1.0 - a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


def rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.linalg.norm(a - ref, axis=-1) / np.linalg.norm(ref, axis=-1)


# ------------------------------------------------------------------ fixtures (seeded, cached, read-only)
POOL_CASES = [(B, g, p) for B in (1, 3) for g in (16, 23) for p in (3.0, 2.5)]
ENCODER_CASES = [(1, 1), (5, 1), (7, 3), (32, 32), (37, 16)]  # (B, group)


@functools.lru_cache(maxsize=None)
def head_sd(seed=0):
    return W.crica_head_state_dict(seed)


@functools.lru_cache(maxsize=None)
def pool_fixture(B, g):
    """(tokens_prenorm f32 [B, 1 + g^2, 768], norm_w, norm_b): a residual stream with a
    per-channel offset and spread (so many normed channels are negative), and patch token 3
    of frame 0 all zero."""
    rng = np.random.default_rng([17, B, g])
    off = rng.standard_normal(E) * 0.5
    spread = np.exp(rng.standard_normal(E) * 0.3)
    x = (rng.standard_normal((B, 1 + g * g, E)) * spread + off).astype(np.float32)
    x[0, 1 + 3] = 0.0
    norm_w = (1.0 + 0.1 * rng.standard_normal(E)).astype(np.float32)
    norm_b = (0.05 * rng.standard_normal(E)).astype(np.float32)
    for a in (x, norm_w, norm_b):
        a.setflags(write=False)
    return x, norm_w, norm_b


@functools.lru_cache(maxsize=None)
def pooled_fixture(B):
    """Pyramid rows f32 [B, 14, 768] with the scales the pool produces: a CLS row of unit
    spread, GeM rows near 768^-1/2 and positive; a shared part plus a per-frame part."""
    rng = np.random.default_rng([23, B])
    shared = rng.standard_normal((1, ROWS, E))
    x = 0.6 * shared + 0.8 * rng.standard_normal((B, ROWS, E))
    x[:, 1:] = np.abs(x[:, 1:]) * 0.036 + 0.004
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def encoder_reference(B, group):
    """(float64 descriptors, e_f32, e_split) of pooled_fixture(B) under head_sd(): the two
    floors are the worst frame's 1 - cos against float64."""
    x, sd = pooled_fixture(B), head_sd()
    ref = encode(x, sd, group)
    e_f32 = max(one_minus_cos(a, b) for a, b in zip(encode(x, sd, group, "f32"), ref))
    e_split = max(one_minus_cos(a, b) for a, b in zip(encode(x, sd, group, "split"), ref))
    ref.setflags(write=False)
    return ref, e_f32, e_split


@functools.lru_cache(maxsize=None)
def e2e_fixture():
    """3 seeded 480 x 640 BGR frames (smooth structure plus noise) and CricaVPRNet weights."""
    rng = np.random.default_rng(29)
    yy, xx = np.mgrid[0:480, 0:640]
    frames = np.empty((3, 480, 640, 3), np.uint8)
    for b in range(3):
        base = [127 + 90 * np.sin(xx / rng.uniform(20, 90) + rng.uniform(0, 6)) * np.cos(yy / rng.uniform(20, 90))
                for _ in range(3)]
        img = np.stack(base, -1) + rng.normal(0, 12, (480, 640, 3))
        frames[b] = np.clip(img, 0, 255).astype(np.uint8)
    frames.setflags(write=False)
    return {"frames": frames, "state_dict": W.crica_state_dict(0)}
