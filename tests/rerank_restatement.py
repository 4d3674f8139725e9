"""The selection rule of mlg_rerank_gate in numpy float64 (test infrastructure only).

CricaVPR.rerank_candidates (place_recognition.py:714-757) for every query row of the kNN
gate's output.  Row i's candidates are its entries s < clamp(count[i], 0, k) with mask[i, s]
set, in emission order.  A query frame (q0 + i) that is not cached keeps its first top_k
candidates unchanged with score = float64(sim).  Otherwise combined = 0.5 float64(sim) +
0.5 float64(cross) for a candidate whose frame is cached and inside [0, F), float64(sim)
for any other; the stable descending rank of an entry is (candidates with a larger score) +
(earlier candidates with an equal score); ranks below top_k are kept, in rank order.
Slots past a row's kept entries hold idx -1, sim 0, cross NaN, score 0.
"""
import numpy as np


def rerank_rows(idx, sim, mask, count, cross, top_k, q0=0, cached=None, F=None):
    """idx int [Q, k], sim f32 [Q, k], mask [Q, k] or None, count [Q]; cross(qframe, j) ->
    float32 cross-correlation score (called for scored entries only); cached bool [F] or
    None (all); F: the bank size (None: every index is inside).

    Returns r_idx int32, r_sim f32, r_cross f32, r_score f64 [Q, top_k], r_count int32 [Q]
    and the number of candidates that were not kept."""
    idx, sim = np.asarray(idx), np.asarray(sim, np.float32)
    Q, k = idx.shape
    r_idx = np.full((Q, top_k), -1, np.int32)
    r_sim = np.zeros((Q, top_k), np.float32)
    r_cross = np.full((Q, top_k), np.nan, np.float32)
    r_score = np.zeros((Q, top_k), np.float64)
    r_count = np.zeros(Q, np.int32)
    dropped = 0
    for i in range(Q):
        cnt = min(max(int(count[i]), 0), k)
        slots = [s for s in range(cnt) if mask is None or mask[i][s]]
        qc = cached is None or bool(cached[q0 + i])
        score = np.zeros(len(slots), np.float64)
        cr = np.full(len(slots), np.nan, np.float32)
        for n, s in enumerate(slots):
            j = int(idx[i, s])
            inside = j >= 0 and (F is None or j < F)
            if qc and inside and (cached is None or bool(cached[j])):
                cr[n] = np.float32(cross(q0 + i, j))
                score[n] = 0.5 * np.float64(sim[i, s]) + 0.5 * np.float64(cr[n])
            else:
                score[n] = np.float64(sim[i, s])
        if qc:
            rank = [int((score > score[n]).sum() + (score[:n] == score[n]).sum()) for n in range(len(slots))]
        else:
            rank = list(range(len(slots)))
        for n, s in enumerate(slots):
            if rank[n] < top_k:
                r_idx[i, rank[n]], r_sim[i, rank[n]] = idx[i, s], sim[i, s]
                r_cross[i, rank[n]], r_score[i, rank[n]] = cr[n], score[n]
        r_count[i] = min(len(slots), top_k)
        dropped += len(slots) - int(r_count[i])
    return r_idx, r_sim, r_cross, r_score, r_count, dropped


def row_candidates(idx, sim, mask, count, i):
    """Row i's candidates as the reference's list [(idx, float(sim)), ...]."""
    k = np.asarray(idx).shape[1]
    cnt = min(max(int(count[i]), 0), k)
    return [(int(idx[i][s]), float(sim[i][s])) for s in range(cnt) if mask is None or mask[i][s]]


def crafted_lists(seed, L=12, D=16):
    """Seeded lists over a bank of 9 small frames, q0 = 1: frames 2 and 5 identical and with
    equal sim in row 0 (an exact tie of the combined score), a row of equal sims, rows with
    count < top_k and count = 0, a count past k, unmasked entries in between, frame 7 (a
    query, row 6, and a candidate) and frame 8 not cached.
    Returns feats, idx, sim, mask, count, q0, cached."""
    rng = np.random.default_rng(seed)
    F, k = 9, 6
    feats = rng.standard_normal((F, L, D)).astype(np.float32)
    feats[5] = feats[2]
    q0, Q = 1, 7
    idx = np.stack([rng.permutation(F)[:k] for _ in range(Q)]).astype(np.int32)
    sim = rng.uniform(0.3, 0.95, (Q, k)).astype(np.float32)
    idx[0] = [2, 7, 5, 8, 0, 3]
    sim[0, 0] = sim[0, 2] = np.float32(0.625)   # the tie: identical features, equal sim
    sim[1, :] = np.float32(0.5)                 # equal sims throughout one row
    count = np.array([k, k, 2, 0, k, 9, k], np.int32)  # 9: clamped to k
    mask = (rng.random((Q, k)) > 0.3).astype(np.uint8)
    mask[0, :4] = 1
    cached = np.ones(F, np.uint8)
    cached[[7, 8]] = 0
    return feats, idx, sim, mask, count, q0, cached
