"""The bf16 GEMM's epilogues that only whole-model runs reached (gemm_bf16.hip: EpiConv,
EpiConvUp, EpiBiasReluBF16, EpiBiasAddRelu, EpiBiasF32, EpiBiasSplitBF16, EpiQKV, EpiPatch,
EpiSimLoFTR, and EpiConv behind the implicit-GEMM convolution), each through its op-level
entry point against a float64 host reference built from the same bf16 values.  GPU only.

Shapes.  The build's default variant picks the kernel from (N, K): (256, 128) is the
persistent k_gemm256 (EpiConv / EpiConvUp run row-staged there), (256, 192) k_gemm<64>,
(128, 64) k_gemm_nt; M = 1 / 255 / 257 / 300 puts a ragged last M-tile against the 128- and
the 256-row tile.  A is a column slice of a buffer K + 64 wide whose other columns are NaN;
every output and residual row is wider than N where the launcher takes a leading dimension,
every output has 8 rows after row M - 1, and everything outside the region the kernel owns
is prefilled (NaN in f32, the bit pattern 0x5A5A in bf16) and must come back untouched.

Exact cases.  Operands are small integers (A rows of at most 128 entries +-1, W in {-1, 0,
1}, integer bias / residual / position rows), so every output is an integer of magnitude
<= 256: the f32 sum and its bf16 rounding are exact in any summation order, and the output
must equal the reference laid out as documented, bit for bit.

Numeric cases.  Tolerances are derived per element (u = 2^-24, the f32 unit roundoff):
  * product: K exact bf16 x bf16 products summed in f32 in an order the MFMA fixes; any
    order's error is at most (K - 1) u S, S = (|A| |W|^T); the bound used is 2 K u S.  The
    split product (EpiSimLoFTR) has 3 K0 terms and S over its three products.
  * one u |value| for every f32 add, multiply or divide of the epilogue (bias, residual,
    LeakyReLU's slope, elu's - 1 and + 1, vdiv, the similarity's two scalings).
  * a bf16 store: 2^-8 |y| (half an ulp of an 8-bit significand), the f32 error before it
    growing by 1 + 2^-8; a hi / lo pair: 2^-16 |y| (the kernel documents 2^-17).
  * elu + 1 (act = 3) calls expf; its slope is at most 1, so the input error passes
    through unchanged.  expf's own error cannot be read off the code: EXPF_REL below is
    twice the largest relative error of the device's f32 exp against float64 exp over
    this file's own pre-activation values (measured: 8.15e-8, 0.68 of an f32 ulp;
    test_expf_term re-measures it on every run and holds it to EXPF_REL).
  * bilinear x2 (EpiConvUp): the f32 source coordinate sh * y carries at most 2 u max(h,
    w) of absolute error and each weight one more u, the nine f32 operations that blend
    the four corners and add the lateral value each at most u times a value bounded by
    max |src| (or the output): (8 max(h, w) + 12) u max |src| + u |out|.
Every numeric case runs 3 times on the same inputs and must give the same bits."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from mlgate import _native

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF16 = 2.0 ** -8
PAIR = 2.0 ** -16
EXPF_MEASURED = 8.15e-8
EXPF_REL = 2.0 * EXPF_MEASURED
RUNS = 3
KERNELS = ((256, 128), (256, 192), (128, 64))  # k_gemm256, k_gemm<64>, k_gemm_nt
MS = (1, 255, 257, 300)
MMAX = 300
APAD = 64   # lda = K + APAD
GUARD = 8   # output rows after row M - 1
SENT16 = 0x5A5A
LEAKY = float(torch.tensor(0.01, dtype=torch.float32).double())  # the kernel's 0.01f


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def S(dev):
    return _native.stream_of(dev)


def L():
    return _native.lib()


def full_range(rows, cols, g, scale):
    """Seeded normal values over 2^-6 .. 2^6 times `scale`, both signs."""
    e = torch.rand(rows, cols, generator=g) * 12.0 - 6.0
    return torch.randn(rows, cols, generator=g) * torch.exp2(e) * scale


def report(name, err, tol):
    ratio = (err / tol.clamp_min(1e-300)).max().item()
    print(f"{name}: max |err| {err.max().item():.3e}, max err / tol {ratio:.3f}")
    return ratio


# ------------------------------------------------------------------ buffers and guards
def strided_a(a, dev):
    """The bf16 operand as columns [32, 32 + K) of a NaN-filled [M, K + 64] device buffer."""
    M, K = a.shape
    buf = torch.full((M, K + APAD), float("nan"), dtype=torch.bfloat16, device=dev)
    buf[:, 32:32 + K] = a.to(dev)
    return buf[:, 32:32 + K]  # keeps buf alive


def out_f32(rows, ld, dev, fill=None):
    """[rows + GUARD, ld] of NaN, `fill` ([rows, n]) in its top-left corner."""
    buf = torch.full((rows + GUARD, ld), float("nan"), device=dev)
    if fill is not None:
        buf[:rows, :fill.shape[1]] = fill.to(dev)
    return buf


def out_bf16(rows, ld, dev):
    return torch.full((rows + GUARD, ld), SENT16, dtype=torch.int16, device=dev).view(torch.bfloat16)


def outside(buf, rows, cols):
    m = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    m[:rows, :cols] = False
    return m


def untouched_f32(buf, rows, cols):
    return bool(torch.isnan(buf[outside(buf, rows, cols)]).all())


def untouched_bf16(buf, rows, cols):
    return bool((buf.view(torch.int16)[outside(buf, rows, cols)] == SENT16).all())


def same_bits(outs):
    """Every run's outputs (tuples of tensors or None) equal the first run's, bit for bit."""
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            if a is not None and not torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                                                 b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)):
                return False
    return True


# ---------------------------------------------------------------------------- problems
@functools.lru_cache(maxsize=None)
def problem(N, K, M=MMAX):
    """Host operands and float64 product of an M-row problem, computed once per (N, K):
    `case` gives every test its first rows, and nothing modifies it."""
    g = torch.Generator().manual_seed(1000 * K + N)
    A = full_range(M, K, g, 1.0).to(torch.bfloat16)
    W = full_range(N, K, g, 1.0 / (64.0 * K ** 0.5)).to(torch.bfloat16)
    a, w = A.double(), W.double()
    return dict(A=A, W=W, prod=a @ w.T, tol=2.0 * K * U * (a.abs() @ w.abs().T),
                bias=torch.randn(N, generator=g) * 0.5, R=torch.randn(M, N, generator=g) * 2.0)


def case(M, N, K):
    return {k: (v[:M] if k in ("A", "prod", "tol", "R") else v) for k, v in problem(N, K).items()}


@functools.lru_cache(maxsize=None)
def exact_problem(N, K, M=MMAX):
    """Integer operands: A rows of min(K, 128) entries +-1 at random columns, W in {-1, 0, 1},
    bias in [-64, 64], residual in [-64, 64]: |product + bias + residual| <= 256."""
    g = torch.Generator().manual_seed(7000 * K + N + M)
    nz = min(K, 128)
    idx = torch.rand(M, K, generator=g).argsort(1)[:, :nz]
    A = torch.zeros(M, K).scatter_(1, idx, torch.randint(0, 2, (M, nz), generator=g).float() * 2 - 1)
    W = torch.randint(-1, 2, (N, K), generator=g).float()
    bias = torch.randint(-64, 65, (N,), generator=g).float()
    R = torch.randint(-64, 65, (M, N), generator=g).float()
    return dict(A=A.to(torch.bfloat16), W=W.to(torch.bfloat16), prod=A.double() @ W.double().T, bias=bias, R=R)


def exact_case(M, N, K):
    return {k: (v[:M] if k in ("A", "prod", "R") else v) for k, v in exact_problem(N, K).items()}


def assert_exact_in_bf16(ref):
    """The reference is its own bf16 rounding (and then its f32 one): no tolerance needed."""
    assert ref.abs().max() <= 256 and torch.equal(ref, ref.round())
    assert torch.equal(ref, ref.to(torch.bfloat16).double())


def bits(x):
    """float64 values exactly representable in bf16 -> their bf16 bit patterns (int16)."""
    return x.contiguous().to(torch.bfloat16).view(torch.int16)


# ------------------------------------------------------------------------- exact: layouts
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", KERNELS)
def test_bias_split_layout_exact(dev, N, K, M):
    """EpiBiasSplitBF16: hi at [n / 16][m][n % 16]; on integers the low plane is all zero."""
    c = exact_case(M, N, K)
    ref = c["prod"] + c["bias"].double()
    assert_exact_in_bf16(ref)
    A, W, b = strided_a(c["A"], dev), c["W"].to(dev), c["bias"].to(dev)
    H = out_bf16(0, N // 16 * M * 16, dev)  # [GUARD, ..]: row 0 is the plane, the rest guard
    Lo = out_bf16(0, N // 16 * M * 16, dev)
    _native.check(L().mlg_op_gemm_bias_split(P(A), K + APAD, P(W), P(b), P(H), P(Lo), M, N, K, S(dev)), "split")
    torch.cuda.synchronize()
    want = bits(ref).view(M, N // 16, 16).permute(1, 0, 2).reshape(-1)
    assert torch.equal(H[0].view(torch.int16).cpu(), want)
    assert torch.count_nonzero(Lo[0].view(torch.int16)) == 0
    assert untouched_bf16(H, 1, H.shape[1]) and untouched_bf16(Lo, 1, Lo.shape[1])


@functools.lru_cache(maxsize=None)
def vit_operands(N, seed):
    """Integer W [N, 768] and bias for the ViT-shaped launchers (K = 768: A rows keep 128
    non-zeros)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1, 2, (N, 768), generator=g).float(), torch.randint(-64, 65, (N,), generator=g).float()


def sparse_rows(M, g):
    idx = torch.rand(M, 768, generator=g).argsort(1)[:, :128]
    return torch.zeros(M, 768).scatter_(1, idx, torch.randint(0, 2, (M, 128), generator=g).float() * 2 - 1)


@pytest.mark.parametrize("B,T,Tpad", [(2, 64, 64), (2, 65, 128), (3, 70, 128)])
def test_qkv_layout_exact(dev, B, T, Tpad):
    """EpiQKV: Q / K at [h][b Tpad + t][d], V^T at [h][key / 64][d][key % 64], key = b Tpad +
    t; the positions t in [T, Tpad) and the guard past each plane keep the sentinel."""
    M, Np = B * T, B * Tpad
    W, bias = vit_operands(2304, 11)
    A = sparse_rows(M, torch.Generator().manual_seed(100 * T + B))
    y = A.double() @ W.double().T + bias.double()
    assert_exact_in_bf16(y)
    n = 12 * Np * 64
    bufs = [torch.full((n + GUARD * 64,), SENT16, dtype=torch.int16, device=dev) for _ in range(3)]
    Ad, Wd, bd = A.to(torch.bfloat16).to(dev), W.to(torch.bfloat16).to(dev), bias.to(dev)
    _native.check(L().mlg_op_gemm_qkv(P(Ad), P(Wd), P(bd), P(bufs[0]), P(bufs[1]), P(bufs[2]), M, T, Tpad, S(dev)),
                  "qkv")
    torch.cuda.synchronize()
    want = []
    for which in range(3):
        rows = torch.full((12, B, Tpad, 64), SENT16, dtype=torch.int16)  # [h][b][t][d]
        rows[:, :, :T] = bits(y[:, 768 * which:768 * (which + 1)]).view(B, T, 12, 64).permute(2, 0, 1, 3)
        rows = rows.view(12, Np, 64)
        if which == 2:
            rows = rows.view(12, Np // 64, 64, 64).transpose(2, 3)  # [h][key / 64][d][key % 64]
        want.append(rows.reshape(-1))
    for name, buf, w in zip("QKV", bufs, want):
        assert torch.equal(buf[:n].cpu(), w), name
        assert bool((buf[n:] == SENT16).all()), name


def test_patch_layout_exact(dev):
    """EpiPatch: token row b (P + 1) + 1 + p = product + bias + pos[1 + p]; the cls rows
    b (P + 1) and the rows after the last image are not written."""
    from mlgate.vit import PATCH_K
    assert PATCH_K == 768
    B, Pn = 3, 37
    M = B * Pn
    W, bias = vit_operands(768, 13)
    g = torch.Generator().manual_seed(17)
    A = sparse_rows(M, g)
    pos = torch.randint(-64, 65, (1 + Pn, 768), generator=g).float()
    y = (A.double() @ W.double().T + bias.double()).view(B, Pn, 768) + pos[1:].double()
    assert_exact_in_bf16(y)
    X = out_f32(B * (Pn + 1), 768, dev)
    Ad, Wd, bd, pd = A.to(torch.bfloat16).to(dev), W.to(torch.bfloat16).to(dev), bias.to(dev), pos.to(dev)
    _native.check(L().mlg_op_gemm_patch(P(Ad), P(Wd), P(bd), P(pd), P(X), M, Pn, PATCH_K, S(dev)), "patch")
    torch.cuda.synchronize()
    got = X[:B * (Pn + 1)].view(B, Pn + 1, 768).cpu()
    assert torch.equal(got[:, 1:].double(), y)
    assert bool(torch.isnan(got[:, 0]).all()) and bool(torch.isnan(X[B * (Pn + 1):]).all())


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K,nvalid,ldc", [(128, 64, 64, 64), (256, 128, 132, 136), (256, 192, 132, 136)])
def test_bias_relu_nvalid_exact(dev, N, K, nvalid, ldc, M):
    """EpiBiasReluBF16: columns >= nvalid are dropped.  With nvalid = ldc = 64 (ResNet's
    call) a dropped column that is written anyway lands in the next row."""
    c = exact_case(M, N, K)
    ref = (c["prod"] + c["bias"].double()).clamp_min(0.0)[:, :nvalid]
    assert_exact_in_bf16(ref)
    A, W, b = strided_a(c["A"], dev), c["W"].to(dev), c["bias"].to(dev)
    C = out_bf16(M, ldc, dev)
    _native.check(L().mlg_op_gemm_bias_relu(P(A), K + APAD, P(W), P(b), P(C), ldc, nvalid, M, N, K, S(dev)), "relu")
    torch.cuda.synchronize()
    assert torch.equal(C[:M, :nvalid].view(torch.int16).cpu(), bits(ref))
    assert untouched_bf16(C, M, nvalid)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", KERNELS)
def test_bias_add_relu_in_place_exact(dev, N, K, M):
    """EpiBiasAddRelu with R == X (ResNet's identity shortcut) and its bf16 copy, both in
    rows of ldx."""
    c = exact_case(M, N, K)
    ref = (c["prod"] + c["bias"].double() + c["R"].double()).clamp_min(0.0)
    assert_exact_in_bf16(ref)
    ldx = N + 8
    A, W, b = strided_a(c["A"], dev), c["W"].to(dev), c["bias"].to(dev)
    X, C = out_f32(M, ldx, dev, c["R"]), out_bf16(M, ldx, dev)
    _native.check(L().mlg_op_gemm_bias_add_relu(P(A), K + APAD, P(W), P(b), P(X), P(X), ldx, P(C), M, N, K, S(dev)),
                  "add_relu")
    torch.cuda.synchronize()
    assert torch.equal(X[:M, :N].cpu().double(), ref)
    assert torch.equal(C[:M, :N].view(torch.int16).cpu(), bits(ref))
    assert untouched_f32(X, M, N) and untouched_bf16(C, M, N)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", KERNELS)
def test_conv_epilogue_in_place_exact(dev, N, K, M):
    """EpiConv with R == X, bias, no activation, the bf16 copy in wider rows (SuperGlue's
    keypoint-encoder call)."""
    c = exact_case(M, N, K)
    ref = c["prod"] + c["bias"].double() + c["R"].double()
    assert_exact_in_bf16(ref)
    ldx, ldc = N + 8, 2 * N
    A, W, b = strided_a(c["A"], dev), c["W"].to(dev), c["bias"].to(dev)
    X, C = out_f32(M, ldx, dev, c["R"]), out_bf16(M, ldc, dev)
    _native.check(L().mlg_op_gemm_conv(P(A), K + APAD, P(W), P(b), P(X), ldx, P(X), ldx, P(C), ldc, 0, 0, M, N, K,
                                       0.0, S(dev)), "conv")
    torch.cuda.synchronize()
    assert torch.equal(X[:M, :N].cpu().double(), ref)
    assert torch.equal(C[:M, :N].view(torch.int16).cpu(), bits(ref))
    assert untouched_f32(X, M, N) and untouched_bf16(C, M, N)


# --------------------------------------------------------------------- numeric: EpiBiasF32
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", KERNELS)
def test_bias_f32_ld(dev, N, K, M):
    """EpiBiasF32 with lda > K and ldc > N."""
    c = case(M, N, K)
    ldc = N + 8
    A, W, b = strided_a(c["A"], dev), c["W"].to(dev), c["bias"].to(dev)
    outs = []
    for _ in range(RUNS):
        C = out_f32(M, ldc, dev)
        _native.check(L().mlg_op_gemm_bias_f32_ld(P(A), K + APAD, P(W), P(b), P(C), ldc, M, N, K, S(dev)), "bias")
        outs.append((C,))
    torch.cuda.synchronize()
    ref = c["prod"] + c["bias"].double()
    C = outs[0][0]
    assert same_bits(outs), "runs on the same inputs differ"
    assert untouched_f32(C, M, N) and torch.isfinite(C[:M, :N]).all()
    err = (C[:M, :N].cpu().double() - ref).abs()
    assert report(f"bias_f32 M={M} N={N} K={K}", err, c["tol"] + U * ref.abs()) <= 1.0


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", KERNELS)
def test_bias_split_pair(dev, N, K, M):
    """EpiBiasSplitBF16 on the wide-range operands: hi + lo is y = product + bias to the
    pair's 2^-16, both planes k-step-major."""
    c = case(M, N, K)
    A, W, b = strided_a(c["A"], dev), c["W"].to(dev), c["bias"].to(dev)
    outs = []
    for _ in range(RUNS):
        H, Lo = out_bf16(0, N * M, dev), out_bf16(0, N * M, dev)
        _native.check(L().mlg_op_gemm_bias_split(P(A), K + APAD, P(W), P(b), P(H), P(Lo), M, N, K, S(dev)), "split")
        outs.append((H, Lo))
    torch.cuda.synchronize()
    assert same_bits(outs), "runs on the same inputs differ"
    H, Lo = outs[0]
    assert untouched_bf16(H, 1, N * M) and untouched_bf16(Lo, 1, N * M)
    rows = lambda t: t[0].view(N // 16, M, 16).permute(1, 0, 2).reshape(M, N).cpu().double()  # noqa: E731
    ref = c["prod"] + c["bias"].double()
    assert report(f"bias_split M={M} N={N} K={K}", (rows(H) + rows(Lo) - ref).abs(),
                  c["tol"] + U * ref.abs() + PAIR * ref.abs()) <= 1.0


# ------------------------------------------------------------------------ numeric: EpiConv
def conv_reference(prod, tol, bias, R, act, act_cols, vdiv=0.0):
    """float64 EpiConv and the per-element bound of its f32 value (module docstring)."""
    N = prod.shape[1]
    y, t = prod.clone(), tol.clone()
    if bias is not None:
        y = y + bias.double()
        t = t + U * y.abs()
    if R is not None:
        y = y + R.double()
        t = t + U * y.abs()
    pre = y.clone()
    a = slice(0, min(act_cols, N))
    if act == 1:
        y[:, a] = y[:, a].clamp_min(0.0)
    elif act == 2:
        y[:, a] = torch.where(y[:, a] > 0, y[:, a], LEAKY * y[:, a])
        t[:, a] = t[:, a] + U * y[:, a].abs()
    elif act == 3:
        ya = y[:, a]
        out = torch.where(ya > 0, ya + 1.0, torch.exp(ya.clamp_max(0.0)))
        # slope <= 1; expf wherever the kernel's y may be <= 0; the - 1 and the + 1 (for y > 0
        # only the + 1: the smaller bound is covered)
        t[:, a] = (t[:, a] + torch.where(ya - t[:, a] <= 0, EXPF_REL * torch.exp(ya.clamp_max(0.0)), 0.0)
                   + U * ((out - 1.0).abs() + out.abs()))
        y[:, a] = out
    if vdiv != 0.0:
        v = slice(min(act_cols, N), N)
        y[:, v] = y[:, v] / vdiv
        t[:, v] = t[:, v] / abs(vdiv) + U * y[:, v].abs()
    return y, t, pre


def run_conv(dev, M, N, K, act, act_cols, use_bias, use_r, outputs, vdiv=0.0, c=None, name="conv"):
    c = c or case(M, N, K)
    ldr, ldx, ldc = N + 8, N + 16, N + 24
    A, W = strided_a(c["A"], dev), c["W"].to(dev)
    b = c["bias"].to(dev) if use_bias else None
    R = out_f32(M, ldr, dev, c["R"]) if use_r else None
    outs = []
    for _ in range(RUNS):
        X = out_f32(M, ldx, dev) if "X" in outputs else None
        C = out_bf16(M, ldc, dev) if "C" in outputs else None
        _native.check(L().mlg_op_gemm_conv(P(A), K + APAD, P(W), P(b), P(R), ldr, P(X), ldx, P(C), ldc, act,
                                           act_cols, M, N, K, vdiv, S(dev)), name)
        outs.append((X, C))
    torch.cuda.synchronize()
    assert same_bits(outs), "runs on the same inputs differ"
    ref, tol, pre = conv_reference(c["prod"], c["tol"], c["bias"] if use_bias else None, c["R"] if use_r else None,
                                   act, act_cols, vdiv)
    X, C = outs[0]
    tag = f"{name} M={M} N={N} K={K} act={act}/{act_cols} bias={int(use_bias)} R={int(use_r)} out={outputs}"
    ratios = []
    if X is not None:
        assert untouched_f32(X, M, N) and torch.isfinite(X[:M, :N]).all()
        ratios.append(report(tag + " f32", (X[:M, :N].cpu().double() - ref).abs(), tol))
    if C is not None:
        assert untouched_bf16(C, M, N) and torch.isfinite(C[:M, :N].float()).all()
        ratios.append(report(tag + " bf16", (C[:M, :N].cpu().double() - ref).abs(),
                             (1.0 + BF16) * tol + BF16 * ref.abs()))
    assert max(ratios) <= 1.0
    return pre


# act, act_cols (None: N), bias, R, outputs: every activation, with and without bias and
# residual, X only / C only / both, and the activation boundary at N, at a wave boundary
# (64) and inside a wave (132; for N = 128 that is past the last column)
CONV_CASES = [(0, None, True, False, "X"), (1, 64, True, True, "XC"), (2, 132, False, True, "C"),
              (3, None, True, False, "XC"), (3, 64, False, False, "X"), (1, 132, False, False, "C"),
              (2, None, True, True, "X"), (3, 132, True, True, "C")]


@pytest.mark.parametrize("cfg", CONV_CASES, ids=lambda c: f"act{c[0]}-cols{c[1]}-b{int(c[2])}-r{int(c[3])}-{c[4]}")
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", KERNELS)
def test_conv_epilogue(dev, N, K, M, cfg):
    act, cols, use_bias, use_r, outputs = cfg
    run_conv(dev, M, N, K, act, N if cols is None else cols, use_bias, use_r, outputs)


@pytest.mark.parametrize("M", MS)
def test_conv_epilogue_elu_vdiv(dev, M):
    """LoFTR's q, k | v projection: elu + 1 on the first 2 N / 3 columns, the rest / 7."""
    run_conv(dev, M, 768, 256, 3, 512, True, False, "XC", vdiv=7.0, name="conv_vdiv")


def test_expf_term(dev):
    """The one bound not derived from the code: the device's f32 exp against float64 exp over
    the pre-activation values the elu cases see (the non-positive ones, where expf runs)."""
    worst = 0.0
    for N, K in KERNELS + ((768, 256),):
        c = case(MMAX, N, K)
        for pre in (c["prod"] + c["bias"].double(), c["prod"], c["prod"] + c["bias"].double() + c["R"].double()):
            y = pre.float().clamp_max(0.0).to(dev)
            rel = ((torch.exp(y).double() - torch.exp(y.double())).abs() / torch.exp(y.double())).max().item()
            worst = max(worst, rel)
    print(f"expf: max relative error {worst:.3e} (recorded {EXPF_MEASURED:.3e}, allowed {EXPF_REL:.3e})")
    assert worst <= EXPF_REL


# ---------------------------------------------------------------------- numeric: EpiConvUp
def upadd_reference(prod, tol, bias, src, B, h, w):
    N = prod.shape[1]
    up = F.interpolate(src.double().view(B, h, w, N).permute(0, 3, 1, 2), scale_factor=2, mode="bilinear",
                       align_corners=True).permute(0, 2, 3, 1).reshape(-1, N)
    lat = prod + bias.double()
    ref = lat + up
    t = tol + U * lat.abs() + (8 * max(h, w) + 12) * U * src.abs().max().item() + U * ref.abs()
    return ref, (1.0 + BF16) * t + BF16 * ref.abs()


@pytest.mark.parametrize("B,h,w", [(2, 5, 7), (1, 1, 3), (1, 3, 1)])
@pytest.mark.parametrize("N,K", KERNELS)
def test_conv_upadd(dev, N, K, B, h, w):
    """EpiConvUp against float64 F.interpolate(x2, bilinear, align_corners=True) + product +
    bias.  (2, 5, 7): M = 280, the second image starts inside the first 256-row tile; h == 1
    and w == 1 are the degenerate scales.  The launcher fixes the row length of C and src at
    N, so only the rows after M - 1 guard the output."""
    M = B * 4 * h * w
    c = case(M, N, K)
    g = torch.Generator().manual_seed(31 * h + w)
    src = torch.randn(B * h * w, N, generator=g) * 2.0
    A, W, b, sd = strided_a(c["A"], dev), c["W"].to(dev), c["bias"].to(dev), src.to(dev)
    outs = []
    for _ in range(RUNS):
        C = out_bf16(M, N, dev)
        _native.check(L().mlg_op_gemm_conv_upadd(P(A), K + APAD, P(W), P(b), P(sd), h, w, P(C), M, N, K, S(dev)),
                      "upadd")
        outs.append((C,))
    torch.cuda.synchronize()
    assert same_bits(outs), "runs on the same inputs differ"
    ref, tol = upadd_reference(c["prod"], c["tol"], c["bias"], src, B, h, w)
    C = outs[0][0]
    assert untouched_bf16(C, M, N) and torch.isfinite(C[:M].float()).all()
    assert report(f"upadd M={M} N={N} K={K} hw={h}x{w}", (C[:M].cpu().double() - ref).abs(), tol) <= 1.0


# -------------------------------------------------------------------- numeric: EpiSimLoFTR
def split_planes(x):
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


@pytest.mark.parametrize("M,ncols,lds,Npad,nb", [(70, 250, 252, 256, 1), (300, 262, 264, 512, 1),
                                                 (300, 262, 264, 512, 2)])
def test_sim_split_loftr(dev, M, ncols, lds, Npad, nb):
    """EpiSimLoFTR: columns < ncols = the three-product split similarity / 256 / 0.1, columns
    [ncols, lds) exactly -inf, nothing at >= lds (rows are lds long, so such a write would
    land in the next row's first elements); nb = 2 is the batched form, the two problems'
    operands pstride apart with a gap between them."""
    K0 = 256
    g = torch.Generator().manual_seed(M + ncols)
    pstride = Npad * 2 * K0 + 1024  # elements: past the larger operand, plus a gap
    Ad = torch.full(((nb - 1) * pstride + M * 2 * K0,), float("nan"), dtype=torch.bfloat16, device=dev)
    Bd = torch.full(((nb - 1) * pstride + Npad * 2 * K0,), float("nan"), dtype=torch.bfloat16, device=dev)
    refs, tols = [], []
    for z in range(nb):
        ah, al = split_planes(full_range(M, K0, g, 1.0))
        bh, bl = split_planes(full_range(Npad, K0, g, 1.0 / 64.0))
        Ad[z * pstride:z * pstride + M * 2 * K0] = torch.cat([ah, al], 1).reshape(-1).to(dev)
        Bd[z * pstride:z * pstride + Npad * 2 * K0] = torch.cat([bh, bl], 1).reshape(-1).to(dev)
        d = [t.double() for t in (ah, al, bh[:ncols], bl[:ncols])]
        prod = d[0] @ d[2].T + d[1] @ d[2].T + d[0] @ d[3].T
        mag = d[0].abs() @ d[2].abs().T + d[1].abs() @ d[2].abs().T + d[0].abs() @ d[3].abs().T
        y = prod / 256.0 / 0.1
        refs.append(y)
        tols.append(2.0 * (3 * K0) * U * mag / 25.6 + 2.0 * U * y.abs())
    ref, tol = torch.cat(refs), torch.cat(tols)
    outs = []
    for _ in range(RUNS):
        Sm = out_f32(nb * M, lds, dev)
        _native.check(L().mlg_op_gemm_sim_split_loftr(P(Ad), P(Bd), M, Npad, K0, P(Sm), lds, ncols, nb, pstride,
                                                      S(dev)), "sim")
        outs.append((Sm,))
    torch.cuda.synchronize()
    Sm = outs[0][0]
    assert all(torch.equal(Sm[:nb * M].view(torch.int32), o[0][:nb * M].view(torch.int32)) for o in outs[1:])
    assert bool(torch.isnan(Sm[nb * M:]).all())
    got = Sm[:nb * M].cpu()
    assert bool((got[:, ncols:] == float("-inf")).all())
    assert torch.isfinite(got[:, :ncols]).all()
    assert report(f"sim_loftr M={M} ncols={ncols} lds={lds} nb={nb}", (got[:, :ncols].double() - ref).abs(), tol) <= 1.0


# ------------------------------------------------------- numeric: the implicit convolution
def test_conv2d_nhwc_epilogue(dev):
    """mlg_op_conv2d_nhwc_epi: the 3 x 3 stride-2 case of test_loftr_gpu's convolution test
    with a residual, ReLU, both outputs and ldr != ldx != ldc != N."""
    B, H, W_, Cin, k, s, N = 2, 61, 79, 128, 3, 2, 256
    Ho, Wo = (H + s - 1) // s, (W_ + s - 1) // s
    M, K = B * Ho * Wo, k * k * Cin
    ldr, ldx, ldc = N + 8, N + 16, N + 24
    g = torch.Generator().manual_seed(5)
    x = full_range(B * H * W_, Cin, g, 1.0).view(B, H, W_, Cin).to(torch.bfloat16)
    w = full_range(N, K, g, 1.0 / (64.0 * K ** 0.5)).view(N, k, k, Cin).to(torch.bfloat16)
    bias, R = torch.randn(N, generator=g) * 0.5, torch.randn(M, N, generator=g) * 2.0
    conv = lambda a, b: F.conv2d(a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2), stride=s,  # noqa: E731
                                 padding=k // 2).permute(0, 2, 3, 1).reshape(M, N)
    prod, mag = conv(x.double(), w.double()), conv(x.double().abs(), w.double().abs())
    ref, tol, _ = conv_reference(prod, 2.0 * K * U * mag, bias, R, 1, N)
    xd, wd, bd = x.to(dev), w.reshape(N, K).contiguous().to(dev), bias.to(dev)
    Rd, zero = out_f32(M, ldr, dev, R), torch.zeros(8, dtype=torch.bfloat16, device=dev)
    outs = []
    for _ in range(RUNS):
        X, C = out_f32(M, ldx, dev), out_bf16(M, ldc, dev)
        _native.check(L().mlg_op_conv2d_nhwc_epi(P(xd), P(zero), B, H, W_, Cin, k, s, P(wd), P(bd), P(Rd), ldr, P(X),
                                                 ldx, P(C), ldc, 1, N, N, S(dev)), "conv2d")
        outs.append((X, C))
    torch.cuda.synchronize()
    assert same_bits(outs), "runs on the same inputs differ"
    X, C = outs[0]
    assert untouched_f32(X, M, N) and untouched_bf16(C, M, N)
    r1 = report("conv2d_epi f32", (X[:M, :N].cpu().double() - ref).abs(), tol)
    r2 = report("conv2d_epi bf16", (C[:M, :N].cpu().double() - ref).abs(), (1.0 + BF16) * tol + BF16 * ref.abs())
    assert max(r1, r2) <= 1.0


# ------------------------------------------------------------------ walking tiles and races
def walking_operands(dev):
    """More 256 x 256 output tiles than CUs, so a k_gemm256 workgroup takes a second tile:
    the row-staged epilogue's LDS image is the stage the next tile's first DMA refills."""
    M, N, K = 256 * 130 + 4, 512, 128
    tiles = ((M + 255) // 256) * (N // 256)
    assert tiles == 262 and tiles > torch.cuda.get_device_properties(dev).multi_processor_count
    g = torch.Generator().manual_seed(77)
    A = full_range(M, K, g, 1.0).to(torch.bfloat16)
    W = full_range(N, K, g, 1.0 / (64.0 * K ** 0.5)).to(torch.bfloat16).to(dev)
    bias = (torch.randn(N, generator=g) * 0.5).to(dev)
    As = strided_a(A, dev)
    a, w = As.double(), W.double()  # the float64 reference on the device
    return M, N, K, As, W, bias, a @ w.T, 2.0 * K * U * (a.abs() @ w.abs().T), g


def test_conv_epilogue_walking_tiles(dev):
    M, N, K, A, W, bias, prod, tol, g = walking_operands(dev)
    ldr, ldx, ldc = N + 8, N + 16, N + 24
    R = torch.randn(M, N, generator=g) * 2.0
    Rd = out_f32(M, ldr, dev, R)
    outs = []
    for _ in range(RUNS):
        X, C = out_f32(M, ldx, dev), out_bf16(M, ldc, dev)
        _native.check(L().mlg_op_gemm_conv(P(A), K + APAD, P(W), P(bias), P(Rd), ldr, P(X), ldx, P(C), ldc, 1, N, M,
                                           N, K, 0.0, S(dev)), "conv")
        outs.append((X, C))
    torch.cuda.synchronize()
    assert same_bits(outs), "runs on the same inputs differ"
    ref, tol, _ = conv_reference(prod, tol, bias, Rd[:M, :N], 1, N)
    X, C = outs[0]
    assert untouched_f32(X, M, N) and untouched_bf16(C, M, N)
    r1 = report("conv walking f32", (X[:M, :N].double() - ref).abs(), tol)
    r2 = report("conv walking bf16", (C[:M, :N].double() - ref).abs(), (1.0 + BF16) * tol + BF16 * ref.abs())
    assert max(r1, r2) <= 1.0


def test_conv_upadd_walking_tiles(dev):
    M, N, K, A, W, bias, prod, tol, g = walking_operands(dev)
    B, h, w = 1, 53, 157
    assert M == B * 4 * h * w
    src = (torch.randn(B * h * w, N, generator=g) * 2.0).to(dev)
    outs = []
    for _ in range(RUNS):
        C = out_bf16(M, N, dev)
        _native.check(L().mlg_op_gemm_conv_upadd(P(A), K + APAD, P(W), P(bias), P(src), h, w, P(C), M, N, K, S(dev)),
                      "upadd")
        outs.append((C,))
    torch.cuda.synchronize()
    assert same_bits(outs), "runs on the same inputs differ"
    ref, tol = upadd_reference(prod, tol, bias, src, B, h, w)
    C = outs[0][0]
    assert untouched_bf16(C, M, N)
    assert report("upadd walking", (C[:M].double() - ref).abs(), tol) <= 1.0


# --------------------------------------------------------------------------------- contracts
def test_launchers_reject_bad_arguments(dev):
    """Each launcher's MLG_EINVAL guard returns before any launch (the buffers are sized for
    the nominal shapes all the same)."""
    M, N, K = 64, 128, 64
    A = torch.zeros(M, K, dtype=torch.bfloat16, device=dev)
    W = torch.zeros(256, K, dtype=torch.bfloat16, device=dev)
    b = torch.zeros(256, device=dev)
    X, C = torch.zeros(M, 256, device=dev), torch.zeros(M, 256, dtype=torch.bfloat16, device=dev)
    s = S(dev)

    def conv(x, c, act):
        return L().mlg_op_gemm_conv(P(A), K, P(W), P(b), None, 0, P(x), N, P(c), N, act, N, M, N, K, 0.0, s)

    assert conv(None, None, 1) == -1      # no output
    assert conv(X, C, 4) == -1            # unknown activation
    assert conv(X, C, 3) == 0
    src = torch.zeros(M * N, device=dev)
    assert L().mlg_op_gemm_conv_upadd(P(A), K, P(W), P(b), P(src), 3, 5, P(C), M, N, K, s) == -1   # 64 % 60
    assert L().mlg_op_gemm_conv_upadd(P(A), K, P(W), P(b), P(src), 2, 2, P(C), M, N, K, s) == 0
    H = torch.zeros(2, 256 * M, dtype=torch.bfloat16, device=dev)
    assert L().mlg_op_gemm_bias_split(P(A), K, P(W), P(b), P(H[0]), P(H[1]), M, 136, K, s) == -1   # N % 16
    assert L().mlg_op_gemm_bias_split(P(A), K, P(W), P(b), P(H[0]), P(H[1]), M, N, K, s) == 0
    A7 = torch.zeros(2 * M, 768, dtype=torch.bfloat16, device=dev)
    W7 = torch.zeros(2304, 768, dtype=torch.bfloat16, device=dev)
    b7 = torch.zeros(2304, device=dev)
    q = torch.zeros(3, 12 * 256 * 64, dtype=torch.bfloat16, device=dev)

    def qkv(T, Tpad):
        return L().mlg_op_gemm_qkv(P(A7), P(W7), P(b7), P(q[0]), P(q[1]), P(q[2]), 2 * M, T, Tpad, s)

    assert qkv(64, 96) == -1              # Tpad % 64
    assert qkv(128, 64) == -1             # Tpad < T
    assert qkv(64, 64) == 0
    A5 = torch.zeros(M, 512, dtype=torch.bfloat16, device=dev)
    B5 = torch.zeros(256, 512, dtype=torch.bfloat16, device=dev)
    Sm = torch.zeros(M, 256, device=dev)

    def sim(lds, ncols):
        return L().mlg_op_gemm_sim_split_loftr(P(A5), P(B5), M, 256, 256, P(Sm), lds, ncols, 1, 0, s)

    assert sim(248, 250) == -1            # ncols > lds
    assert sim(250, 250) == -1            # lds % 4
    assert sim(252, 250) == 0
    torch.cuda.synchronize()
