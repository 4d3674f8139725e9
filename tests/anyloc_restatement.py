"""float64 numpy restatement of AnyLoc's native branch (csrc/vlad.hip, mlgate/anyloc.py):
hard-assignment VLAD as upstream AnyLoc's VLAD(norm_descs=True, vlad_mode='hard',
intra_norm=True) and the Lloyd loop that fits its vocabulary, plus float32 variants with
another summation order whose distance to the float64 results is the rounding floor the
GPU tests scale their bars by (e_f32).  All bars and margins in tests/test_anyloc_*.py are
computed from these functions, never from what the kernels return."""
import numpy as np

D = 768
EPS = 1e-12


def unit(x):
    x = np.asarray(x, np.float64)
    return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), EPS)


def cosines(tokens, centers):
    """[P, K] float64: x^_i . c^_k."""
    return unit(tokens) @ unit(centers).T


def assign(tokens, centers):
    """labels (argmax, lowest k on ties), the top-2 cosine gap and the second-best cluster per token."""
    s = cosines(tokens, centers)
    labels = np.argmax(s, axis=1)  # first maximum: the lowest k
    order = np.argsort(-s, axis=1, kind="stable")
    rows = np.arange(len(s))
    second = np.where(order[:, 0] == labels, order[:, 1], order[:, 0])
    gap = s[rows, labels] - s[rows, second]
    return labels.astype(np.int32), gap, second.astype(np.int32)


def vlad(tokens, centers, labels=None):
    """One frame: tokens [P, 768], centres [K, 768] -> float64 [K * 768] (steps 1-6)."""
    c = np.asarray(centers, np.float64)
    xh = unit(tokens)
    if labels is None:
        labels = assign(tokens, centers)[0]
    V = np.zeros_like(c)
    for k in range(len(c)):
        m = np.flatnonzero(labels == k)
        if len(m):
            V[k] = (xh[m] - c[k]).sum(axis=0)  # residual against the stored centre
    V /= np.maximum(np.linalg.norm(V, axis=1, keepdims=True), EPS)
    v = V.reshape(-1)
    return v / max(np.linalg.norm(v), EPS)


def vlad_f32(tokens, centers, labels):
    """The same in float32 throughout, members summed in descending token order (the kernels
    and vlad() sum ascending): its 1 - cos to vlad() is the float32 rounding floor e_f32."""
    f = np.float32
    x = np.asarray(tokens, f)
    c = np.asarray(centers, f)
    n = np.sqrt(np.sum(x * x, axis=1, dtype=f), dtype=f)
    xh = x / np.maximum(n, f(EPS))[:, None]
    V = np.zeros_like(c)
    for k in range(len(c)):
        m = np.flatnonzero(labels == k)[::-1]
        if len(m):
            V[k] = np.add.reduce(xh[m] - c[k], axis=0, dtype=f)
    V = V / np.maximum(np.sqrt(np.sum(V * V, axis=1, dtype=f), dtype=f), f(EPS))[:, None]
    v = V.reshape(-1)
    return v / np.maximum(np.sqrt(np.sum(v * v, dtype=f), dtype=f), f(EPS))


def one_minus_cos(a, b):
    """1 - cos as |a^ - b^|^2 / 2 in float64: no cancellation at the 1e-15 level the float32
    floor lives at (1 - a.b loses it to float64 rounding)."""
    a, b = unit(a), unit(b)
    d = a - b
    return 0.5 * np.sum(d * d, axis=-1)


def kmeans_update(xh, labels, prev):
    """Means of the assigned unit tokens; an empty cluster keeps its previous centre."""
    c = np.array(prev, np.float64)
    for k in range(len(c)):
        m = np.flatnonzero(labels == k)
        if len(m):
            c[k] = xh[m].sum(axis=0) / len(m)
    return c


def kmeans_update_f32(tokens, labels, prev):
    """kmeans_update in float32, members summed in descending order: the centres' rounding floor."""
    f = np.float32
    x = np.asarray(tokens, f)
    n = np.sqrt(np.sum(x * x, axis=1, dtype=f), dtype=f)
    xh = x / np.maximum(n, f(EPS))[:, None]
    c = np.array(prev, f)
    for k in range(len(c)):
        m = np.flatnonzero(labels == k)[::-1]
        if len(m):
            c[k] = np.add.reduce(xh[m], axis=0, dtype=f) / f(len(m))
    return c


def kmeans(tokens, num_clusters, seed=0, max_iter=100):
    """The Lloyd loop of mlgate.anyloc.fit_vocabulary: initial centres the unit tokens at
    default_rng(seed).choice(M, K, replace=False); each step assigns against the current
    centres, counts the labels that moved (all of them at the first step) and replaces the
    centres by the cluster means; it stops after the step in which no label moved, or
    after max_iter steps.  Returns centres, labels, the number of steps, and the smallest
    top-2 cosine gap any token had at any step."""
    xh = unit(tokens)
    M = len(xh)
    centers = xh[np.random.default_rng(seed).choice(M, num_clusters, replace=False)].copy()
    labels = np.full(M, -1, np.int32)
    n_iter, min_gap = 0, np.inf
    while n_iter < max_iter:
        new, gap, _ = assign(xh, centers)
        min_gap = min(min_gap, float(gap.min()))
        changed = int(np.sum(new != labels))
        labels = new
        centers = kmeans_update(xh, labels, centers)
        n_iter += 1
        if changed == 0:
            break
    return centers, labels, n_iter, min_gap


# ------------------------------------------------------------------- fixtures
HEAD_SHAPES = [(1, 1, 16), (3, 63, 128), (2, 65, 64), (3, 1368, 64)]  # (B, P, K)
GAP_DECIDED = 1e-5  # labels must agree where the float64 top-2 gap is at least this
UNDECIDED_CAP = 0.005


def head_fixture(shape, seed=1):
    """Seeded unit-Gaussian tokens [B, P, 768] and centres [K, 768] of norm ~0.87 (what
    k-means over unit tokens produces), float32.  Where P > 1, token 1 of frame 0 is zero."""
    B, P, K = shape
    rng = np.random.default_rng([seed, B, P, K])
    tokens = rng.standard_normal((B, P, D)).astype(np.float32)
    centers = (rng.standard_normal((K, D)) * (0.87 / np.sqrt(D))).astype(np.float32)
    if P > 1:
        tokens[0, 1] = 0.0
    return tokens, centers


KMEANS_SEED = 0


def planted_mixture(seed=6, M=2000, directions=16, noise=0.07, init_seed=KMEANS_SEED):
    """M tokens around 16 orthogonal directions (direction + noise * N(0, I), a random
    positive scale each).  The tokens fit_vocabulary(seed=init_seed) draws as initial centres
    are given one direction each, so no direction starts split between two centres -- split
    directions put tokens within 1e-5 of a tie.  With these parameters some labels still move
    in the second step (3 steps in all) and no token ever comes within 1e-3 of a tie
    (tests/test_anyloc_cpu.py asserts both)."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((D, directions)))
    which = rng.integers(0, directions, M)
    which[np.random.default_rng(init_seed).choice(M, directions, replace=False)] = np.arange(directions)
    x = q.T[which] + noise * rng.standard_normal((M, D))
    x *= rng.uniform(0.5, 2.0, (M, 1))
    return x.astype(np.float32)


KMEANS_MIN_GAP = 1e-3


# ------------------------------------------------- end to end against the fp32 oracle
E2E_GAP = 1e-4        # F: tokens whose float64 top-2 gap is below this may be assigned either way
E2E_F_CAP = 0.01      # |F| <= 1 % of the frame's tokens
E2E_VOCAB_SEED = 1   # seeds 0 and 1 keep |F| under the cap; seed 2 leaves a one-token cluster whose block is rounding noise
E2E_VOCAB_ITERS = 100
_e2e = {}


def e2e_fixture():
    """Three seeded 480 x 640 noise frames, their fp32 oracle tokens [3, 1368, 768] (seeded synthetic
    DINOv2 weights), a K = 64 vocabulary fitted on those tokens by kmeans() above, and for
    frame 0 the float64 labels, gaps, second-best clusters, the oracle descriptor, e_f32
    and e_flip (the 1 - cos between the oracle descriptor and the one with every token of
    F moved to its second-best cluster).  Computed once per process."""
    if _e2e:
        return _e2e
    import torch
    from mlgate.weights import synthetic_state_dict
    from oracle import vit as ovit
    frames = np.random.default_rng(1).integers(0, 256, (3, 480, 640, 3), dtype=np.uint8)
    sd = synthetic_state_dict(0)
    osd = {k: torch.from_numpy(v) for k, v in sd.items()}
    with torch.no_grad():
        toks = np.stack([ovit.forward_tokens(ovit.preprocess(f, 518, swap_rb=False), osd)[0, 1:].numpy()
                         for f in frames])
    centers = kmeans(toks.reshape(-1, D), 64, E2E_VOCAB_SEED, E2E_VOCAB_ITERS)[0].astype(np.float32)
    labels, gap, second = assign(toks[0], centers)
    F = gap < E2E_GAP
    ref = vlad(toks[0], centers, labels)
    flipped = vlad(toks[0], centers, np.where(F, second, labels))
    _e2e.update(frames=frames, state_dict=sd, tokens=toks, centers=centers, labels=labels, gap=gap, F=F, ref=ref,
                e_f32=float(one_minus_cos(vlad_f32(toks[0], centers, labels), ref)),
                e_flip=float(one_minus_cos(flipped, ref)))
    return _e2e
