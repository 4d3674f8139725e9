"""The sequence-consistency rule of mlg_seq_gate (include/mlgate.h states it; the words here
are the header's) restated in numpy float64, and the synthetic walk its tests run on.  Plain
numpy: no device, no native library."""
import numpy as np

ALIASES = ((44, 20), (52, 37), (75, 1), (90, 38))  # (frame, the place it looks like for that one frame)
ORDER = list(range(40)) + list(range(5, 33)) + list(range(30, 2, -1))  # outward, forward revisit, reverse revisit
FORWARD, REVERSE = range(40, 68), range(68, 96)  # the frames of the two revisiting legs
MIN_GAP, RETRIEVAL_THR, K, W, SEQ_THR = 5.0, 0.5, 5, 3, 0.3


def walk(D, seed=0):
    """(X f32 [96, D], t f64 [96], place [96]): 64 unit-variance Gaussian places of width D,
    visited in ORDER with 0.35 noise per frame; the ALIASES frames show another place."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((64, D))
    place = np.array(ORDER)
    X = G[place] + 0.35 * rng.standard_normal((len(place), D))
    for f, p in ALIASES:
        X[f] = G[p] + 0.35 * rng.standard_normal(D)
    return X.astype(np.float32), np.arange(len(place), dtype=np.float64), place


def similarity64(X):
    """S(a, b) from the descriptors alone, in float64: rows x / (||x|| + 1e-8), S = Xn Xn^T."""
    X = np.asarray(X, np.float64)
    Xn = X / (np.linalg.norm(X, axis=1, keepdims=True) + 1e-8)
    return Xn @ Xn.T


def knn_lists(S, t, min_gap, thr, k):
    """The retrieval's lists from a similarity matrix: per row, |t_j - t_i| < min_gap masked,
    top-k by (similarity descending, index descending), entries below thr dropped.
    Returns idx int32 [N, k], sim f32 [N, k], count int32 [N]."""
    N = len(S)
    idx, sim, count = np.zeros((N, k), np.int32), np.zeros((N, k), np.float32), np.zeros(N, np.int32)
    for i in range(N):
        ok = [j for j in range(N) if not abs(t[j] - t[i]) < min_gap]
        ok.sort(key=lambda j: (-S[i, j], -j))
        top = [j for j in ok[:k] if not S[i, j] < thr]
        idx[i, :len(top)], sim[i, :len(top)], count[i] = top, S[i, top], len(top)
    return idx, sim, count


def seq_rows(S, t, code, has, idx, sim, mask, count, w, min_gap, min_terms, threshold, q0=0):
    """The rule over a similarity table S [N, N] (S[a, b] = S(a, b)): returns s_score f64,
    s_dir int8, s_terms int32, keep uint8 -- all [Q, k] -- and the judged-and-rejected total."""
    N = len(t)
    Q, k = idx.shape
    s_score, s_dir = np.zeros((Q, k), np.float64), np.zeros((Q, k), np.int8)
    s_terms, keep = np.zeros((Q, k), np.int32), np.zeros((Q, k), np.uint8)
    rejected = 0

    def same_floor(x, base):
        return (not has[x]) or (not has[base]) or code[x] == code[base]

    for r in range(Q):
        i = q0 + r
        for s in range(min(max(int(count[r]), 0), k)):
            j = int(idx[r, s])
            if (mask is not None and mask[r, s] == 0) or not 0 <= j < N:
                continue  # not a candidate: zeros
            centre = np.float64(sim[r, s])
            per_dir = {}
            for dr in (1, -1):
                total, n = np.float64(0.0), 0
                for d in range(-w, w + 1):  # ascending
                    a, b = i + d, j + dr * d
                    if d == 0 or not (0 <= a < N and 0 <= b < N):
                        continue
                    if abs(t[a] - t[b]) < min_gap:
                        continue
                    if not (same_floor(a, i) and same_floor(b, j)):
                        continue
                    total = total + np.float64(S[a, b])
                    n += 1
                per_dir[dr] = ((centre + total) / np.float64(1 + n), n)
            eligible = [dr for dr in (1, -1) if per_dir[dr][1] >= min_terms]
            if not eligible:  # kept unjudged
                s_score[r, s], keep[r, s] = centre, 1
                continue
            dr = eligible[0]
            if len(eligible) == 2 and per_dir[-1][0] > per_dir[1][0]:  # +1 on a tie
                dr = -1
            s_score[r, s], s_terms[r, s] = per_dir[dr]
            s_dir[r, s] = dr
            keep[r, s] = 1 if s_score[r, s] >= threshold else 0
            rejected += 1 - int(keep[r, s])
    return s_score, s_dir, s_terms, keep, rejected


def seq_workspace_bytes(N, D, Q, k):
    """include/mlgate.h's layout of mlg_seq_gate's workspace, restated: the normalised
    descriptors f32 [N, D], rounded up to 256 bytes; 0 for a shape the call refuses."""
    if N <= 0 or D <= 0 or Q <= 0 or not 1 <= k <= 64 or Q * k > 2**31 - 1:
        return 0
    return (4 * N * D + 255) // 256 * 256
