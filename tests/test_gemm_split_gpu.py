"""The split-bf16 GEMM (gemm_bf16.hip dma::k_gemm256s) through its op-level entry points,
at the shapes where its K-loop pipeline can go wrong, against a float64 host reference
built from the same bf16 planes.  GPU only.

Shapes: K0 = 64 is one loop iteration (the prologue meets the drain), 128 and 192 give
two and three, 768 is the ViT's own; M = 1 / 255 / 256 / 257 / 530 puts the ragged last
M-tile on every side of the 256-row tile; N = 256 and 768 are one and three N-tiles.  The
walking case has more output tiles than the device has CUs, so that a workgroup hands
over to a second tile while the first one's last K-steps run.

Tolerances (derived, not tuned; u = 2^-24, the f32 unit roundoff):
  * product: the kernel adds n = 3 K0 exact bf16 x bf16 products per element in f32, in an
    order the MFMA fixes.  Any order's error is at most (n - 1) u S, with S the sum of the
    terms' magnitudes; the bound used is 2 n u S, S = |A_hi||W_hi|^T + |A_lo||W_hi|^T +
    |A_hi||W_lo|^T.
  * residual epilogue, x + g (p + b): one rounding each for y = p + b, z = g y and x + z
    (2 u |z| + u |out|, doubled), and the product's bound scaled by |g|.
  * GELU pair epilogue: GELU's slope is at most 1.13, so the input error (product bound +
    u |y|) grows by that; common.h gelu_poly2 documents |error| <= 1e-6 inside +-4.5 and
    <= 3.4e-6 |y| beyond; the pair hi + lo represents its value to 2^-16 relative.
Race screen: every shape runs 20 times in one process on the same inputs and must give
the same bits each time."""
import ctypes
import functools

import pytest
import torch

from mlgate import _native

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
RUNS = 20
MMAX = 530
K0S = (64, 128, 192, 768)
MS = (1, 255, 256, 257, 530)
NS = (256, 768)


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def split_planes(x):
    """[hi | lo] bf16 rows of a float32 matrix: hi = bf16(x), lo = bf16(x - hi)."""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi, lo


def full_range(rows, cols, g, scale):
    """Seeded normal values over 2^-6 .. 2^6 times `scale`, both signs."""
    e = torch.rand(rows, cols, generator=g) * 12.0 - 6.0
    return torch.randn(rows, cols, generator=g) * torch.exp2(e) * scale


@functools.lru_cache(maxsize=None)
def problem(M, N, K0):
    """Host operands and the float64 reference of an M-row problem, computed once: `case`
    below gives every test of the same (N, K0) its first rows, and nothing modifies it."""
    g = torch.Generator().manual_seed(1000 * K0 + N)
    ah, al = split_planes(full_range(M, K0, g, 1.0))
    wh, wl = split_planes(full_range(N, K0, g, 1.0 / (64.0 * K0 ** 0.5)))
    d = [t.double() for t in (ah, al, wh, wl)]
    prod = d[0] @ d[2].T + d[1] @ d[2].T + d[0] @ d[3].T
    mag = d[0].abs() @ d[2].abs().T + d[1].abs() @ d[2].abs().T + d[0].abs() @ d[3].abs().T
    bias = torch.randn(N, generator=g) * 0.5
    gamma = torch.randn(N, generator=g)
    x0 = torch.randn(M, N, generator=g) * 2.0
    return dict(A=torch.cat([ah, al], 1).contiguous(), W=torch.cat([wh, wl], 1).contiguous(), prod=prod,
                tol=2.0 * (3 * K0) * U * mag, bias=bias, gamma=gamma, x0=x0)


def case(M, N, K0):
    p = problem(max(M, MMAX), N, K0)
    return {k: (v[:M] if k in ("A", "prod", "tol", "x0") else v) for k, v in p.items()}


def report(name, err, tol):
    ratio = (err / tol.clamp_min(1e-300)).max().item()
    print(f"{name}: max |err| {err.max().item():.3e}, max err / tol {ratio:.3f}")
    return ratio


def run_residual(dev, M, N, K0):
    c = case(M, N, K0)
    A, W, b, gam, x0 = (c[k].to(dev) for k in ("A", "W", "bias", "gamma", "x0"))
    s = _native.stream_of(dev)
    outs = []
    for _ in range(RUNS):
        X = x0.clone()
        _native.check(_native.lib().mlg_op_gemm_residual_split(P(A), P(W), P(b), P(gam), P(X), M, N, K0, s), "res")
        outs.append(X)
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0], o) for o in outs[1:]), "runs on the same inputs differ"
    g64, y = c["gamma"].double(), c["prod"] + c["bias"].double()
    z = g64 * y
    ref = c["x0"].double() + z
    tol = g64.abs() * (c["tol"] + U * y.abs()) + 2.0 * U * (2.0 * z.abs() + ref.abs())
    err = (outs[0].cpu().double() - ref).abs()
    assert torch.isfinite(outs[0]).all()
    assert report(f"residual M={M} N={N} K0={K0}", err, tol) <= 1.0


def run_bias_gelu(dev, M, N, K0):
    c = case(M, N, K0)
    A, W, b = (c[k].to(dev) for k in ("A", "W", "bias"))
    s = _native.stream_of(dev)
    outs = []
    for _ in range(RUNS):
        C = torch.full((M, 2 * N), float("nan"), dtype=torch.bfloat16, device=dev)
        _native.check(_native.lib().mlg_op_gemm_bias_gelu_split(P(A), P(W), P(b), P(C), M, N, K0, s), "gelu")
        outs.append(C)
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0].view(torch.int16), o.view(torch.int16)) for o in outs[1:]), \
        "runs on the same inputs differ"
    y = c["prod"] + c["bias"].double()
    ref = 0.5 * y * (1.0 + torch.erf(y / 2.0 ** 0.5))
    tol = 1.13 * (c["tol"] + U * y.abs()) + 1e-6 + 3.4e-6 * y.abs() + 2.0 ** -16 * ref.abs()
    out = outs[0].cpu()
    assert torch.isfinite(out.float()).all()
    got = out[:, :N].double() + out[:, N:].double()
    assert report(f"bias_gelu M={M} N={N} K0={K0}", (got - ref).abs(), tol) <= 1.0


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K0", K0S)
def test_residual_split(dev, K0, M, N):
    run_residual(dev, M, N, K0)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K0", K0S)
def test_bias_gelu_split(dev, K0, M, N):
    run_bias_gelu(dev, M, N, K0)


def walking_shape(dev):
    M, N, K0 = 256 * 90, 768, 64
    tiles = (M // 256) * (N // 256)
    assert tiles == 270 and tiles > torch.cuda.get_device_properties(dev).multi_processor_count
    return M, N, K0


def test_residual_split_walking_tiles(dev):
    """270 output tiles on fewer CUs: a workgroup takes a second tile, whose first K-steps
    are prefetched during the last K-steps of the first."""
    run_residual(dev, *walking_shape(dev))


def test_bias_gelu_split_walking_tiles(dev):
    run_bias_gelu(dev, *walking_shape(dev))
