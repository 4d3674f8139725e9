"""Device-resident all-keyframes retrieval: cosine kNN + time mask + threshold + floor gate.

Thin host wrapper over ``mlg_knn_gate`` (include/mlgate.h), which replaces
SemanticPlaceRecognition.find_loop_closures (place_recognition.py:851-911) and
BasePlaceRecognition.compute_all_pairwise_similarities (:179-190).
"""
import numpy as np

from . import _native

# k <= 32: fused scan; <= 256: per-lane lists; beyond: radix select in windows of 4096 ranks
# (knn.hip k_topk_large) -- no upper limit, as the reference's argsort()[:k] has none


def knn_gate(desc, t, floor, has_floor, min_gap, thr, k, gating, q0=0, Q=None, totals=None):
    """desc f32 [N, D], t f64 [N], floor i64 [N], has_floor u8 [N] -- all on the device.
    The threshold compares against float32 similarities in float32 (NumPy >= 2 / NEP 50
    semantics of the reference's ``similarities[j] < self.similarity_threshold``).

    Returns device tensors idx int32 [Q, k], sim f32 [Q, k], valid uint8 [Q, k], count int32 [Q].
    """
    if k < 1:
        raise ValueError(f"k must be >= 1 (got {k})")
    N = desc.shape[0]
    Q = N - q0 if Q is None else Q
    return _native.ops().knn_gate(desc, t, floor, has_floor, float(min_gap), float(thr), int(k), bool(gating),
                                  int(q0), int(Q), totals)


class StreamingKnn:
    """knn_gate as keyframes arrive (mlg_knn_append; include/mlgate.h states the rule): after
    any sequence of appends, ``lists()`` holds bit for bit what ``knn_gate`` returns on the
    keyframes appended so far.  Owns the device state, sized to ``capacity`` rows: the
    normalised descriptors, the timestamps and floor codes, and the per-row lists."""

    def __init__(self, capacity, D, k, min_gap, thr, gating, device="cuda"):
        import torch
        if capacity < 1:
            raise ValueError(f"capacity must be >= 1 (got {capacity})")
        if not 1 <= k <= 32:
            raise ValueError(f"StreamingKnn takes k in [1, 32] (got {k})")
        if D < 4 or D % 4:
            raise ValueError(f"StreamingKnn takes D % 4 == 0 (got {D})")
        self.capacity, self.D, self.k = int(capacity), int(D), int(k)
        self.min_gap, self.thr, self.gating = float(min_gap), float(thr), bool(gating)
        self.n = 0
        dev = torch.device(device)
        self.xn = torch.zeros(self.capacity, self.D, dtype=torch.float32, device=dev)
        self.t = torch.zeros(self.capacity, dtype=torch.float64, device=dev)
        self.floor = torch.zeros(self.capacity, dtype=torch.int64, device=dev)
        self.has_floor = torch.zeros(self.capacity, dtype=torch.uint8, device=dev)
        self.idx = torch.full((self.capacity, self.k), -1, dtype=torch.int32, device=dev)
        self.sim = torch.zeros(self.capacity, self.k, dtype=torch.float32, device=dev)
        self.valid = torch.zeros(self.capacity, self.k, dtype=torch.uint8, device=dev)
        self.count = torch.zeros(self.capacity, dtype=torch.int32, device=dev)

    def append(self, desc_new, t_new, floor_new, has_new):
        """desc_new f32 [B, D] (raw descriptors), t_new f64 [B], floor_new i64 [B], has_new u8
        [B], on the device.  Normalises the new rows into place, updates every list, and
        returns the device tensors (inserted int32 [n_old], evicted_idx int32 [n_old, k],
        n_evicted int32 [n_old]) of the rows that were there before.  No host sync."""
        B = desc_new.shape[0]
        if desc_new.dim() != 2 or desc_new.shape[1] != self.D or B < 1:
            raise ValueError(f"desc_new must be [B >= 1, {self.D}] (got {tuple(desc_new.shape)})")
        if not (t_new.numel() == B and floor_new.numel() == B and has_new.numel() == B):
            raise ValueError(f"t_new / floor_new / has_new must each hold {B} entries (got {t_new.numel()}, "
                             f"{floor_new.numel()}, {has_new.numel()})")
        n_old, n_new = self.n, self.n + B
        if n_new > self.capacity:
            raise ValueError(f"appending {B} keyframes to {n_old} exceeds the capacity {self.capacity}")
        ops = _native.ops()
        self.xn[n_old:n_new] = ops.row_normalize(desc_new.contiguous())
        self.t[n_old:n_new] = t_new.reshape(-1)
        self.floor[n_old:n_new] = floor_new.reshape(-1)
        self.has_floor[n_old:n_new] = has_new.reshape(-1)
        out = ops.knn_append(self.xn, self.t, self.floor, self.has_floor, self.idx, self.sim, self.valid, self.count,
                             n_old, n_new, self.min_gap, self.thr, self.k, self.gating)
        self.n = n_new
        return out

    def lists(self):
        """Views (idx int32 [n, k], sim f32 [n, k], valid uint8 [n, k], count int32 [n]) of the
        state, in knn_gate's layout."""
        n = self.n
        return self.idx[:n], self.sim[:n], self.valid[:n], self.count[:n]


def pairwise_similarities(desc):
    """Device float32 N x N cosine similarity matrix (compute_all_pairwise_similarities)."""
    ops = _native.ops()
    xn = ops.row_normalize(desc)
    return ops.similarity(xn, xn)


def similarity(A, B):
    """Cosine similarities S[Q, N] between the rows of A [Q, D] and B [N, D] (device, float32)."""
    ops = _native.ops()
    return ops.similarity(ops.row_normalize(A), ops.row_normalize(B))


def flatten_matches(idx, sim, valid, count, q0=0):
    """Host flat arrays (q, m, sim, valid) in emission order from per-row device outputs."""
    idx, sim, valid, count = (x.cpu().numpy() for x in (idx, sim, valid, count))
    sel = np.arange(idx.shape[1])[None, :] < count[:, None]
    q = np.repeat(np.arange(q0, q0 + len(count)), count)
    return q, idx[sel].astype(np.int64), sim[sel], valid[sel].astype(bool)


def knn_query(db, qdesc, t_db, t_query, min_gap, k):
    """BasePlaceRecognition.query on the device: db f32 [N, D], qdesc f32 [Q, D], t_db f64 [N],
    t_query f64 [Q] (NaN = no timestamp).  Returns device idx int32 [Q, k], sim f32 [Q, k], count [Q]."""
    if k < 1:
        raise ValueError(f"k must be >= 1 (got {k})")
    return _native.ops().knn_query(db, qdesc, t_db, t_query, float(min_gap), int(k))


def rerank_gate(feats, idx, sim, mask, count, top_k, q0=0, cached=None, totals=None):
    """CricaVPR.rerank_candidates (place_recognition.py:714-757) for every query row of
    knn_gate's output, on the device and asynchronous on the current stream
    (mlg_rerank_gate).  feats f32 [F, L, D]: the local features of the bank frames, query
    row i being frame q0 + i; idx / sim [Q, k], count [Q] as knn_gate returned them; mask
    uint8 [Q, k] (or None: every emitted entry): the entries that are candidates; cached
    uint8 [F] (or None: all) marks the frames whose features are cached; totals int64 [1]
    (or None) is added the number of candidates that were not kept.

    Returns device tensors r_idx int32, r_sim f32 (the global similarity), r_cross f32 (NaN
    where the entry was not scored), r_score f64 -- all [Q, top_k], each row in re-ranked
    order -- and r_count int32 [Q]."""
    k = idx.shape[1]
    if not 1 <= k <= 64:
        raise ValueError(f"rerank_gate takes k in [1, 64] (got {k})")
    if not 1 <= top_k <= k:
        raise ValueError(f"top_k must be in [1, k = {k}] (got {top_k})")
    return _native.ops().rerank_gate(feats, idx, sim, mask, count, int(top_k), int(q0), cached, totals)


def sequence_gate(desc, t, floor, has_floor, idx, sim, mask, count, radius, threshold, min_gap, min_terms=2, q0=0,
                  totals=None):
    """The sequence-consistency check of knn_gate's candidates, on the device and asynchronous
    on the current stream (mlg_seq_gate; include/mlgate.h states the rule).  desc f32 [N, D],
    t f64 [N], floor i64 [N], has_floor u8 [N] as knn_gate takes them; idx / sim [Q, k],
    count [Q] as it returned them, query row r being frame q0 + r; mask uint8 [Q, k] (or None:
    every emitted entry): the entries that are candidates; min_gap: the retrieval's; totals
    int64 [1] (or None) is added the number of judged-and-rejected candidates.

    Returns device tensors s_score f64, s_dir int8, s_terms int32, keep uint8 -- all [Q, k] in
    emission order, nothing compacted."""
    k = idx.shape[1]
    if not 1 <= k <= 64:
        raise ValueError(f"sequence_gate takes k in [1, 64] (got {k})")
    if not 1 <= int(radius) <= 7:
        raise ValueError(f"radius must be in [1, 7] (got {radius})")
    if int(min_terms) < 1:
        raise ValueError(f"min_terms must be >= 1 (got {min_terms})")
    return _native.ops().seq_gate(desc, t, floor, has_floor, idx, sim, mask, count, int(radius), float(threshold),
                                  float(min_gap), int(min_terms), int(q0), totals)


def xcorr_score(qf, mf):
    """CricaVPR.compute_cross_correlation_score on device float32 [n1, D] / [n2, D] -> device scalar."""
    return _native.ops().xcorr_score(qf.contiguous(), mf.contiguous())
