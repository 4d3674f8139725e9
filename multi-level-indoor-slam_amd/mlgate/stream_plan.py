"""StreamingGate's host plan: the floor codes as labels arrive, the format of the changed-rows
transfer, which ordered pairs are live, which are new and bound for the verifier, which were
evicted, what every verified pair's result was, and the cumulative counts.  numpy only -- no
device, no native library -- so every decision here is checked on the CPU
(tests/test_stream_plan_cpu.py); mlgate.pipeline runs the device work this plan drives.  The
batch rules are not restated: the floor coder, the pairs, the verifier's floor skip and the
canonical orientation come from gate_plan.
"""
import numpy as np

from . import gate_plan
from .gate_plan import FloorCoder

COUNT_KEYS = ("matches", "retrieval_floor_rejected", "skipped_floor_mismatch", "verifier_invalid",
              "gate_rejected_cross_floor", "pairs_verified", "verified_valid", "accepted")


# The changed rows of an append come to the host in one int32 transfer whose columns are
# these, in this order: (name, wide) with wide = k columns ([R, k]), else one ([R]).  sim
# travels as its float32 bits.
PACKED_COLUMNS = (("idx", True), ("sim", True), ("valid", True), ("count", False), ("n_evicted", False),
                  ("evicted", True), ("kp_count", False))


def unpack(packed, k):
    """The transfer (int32 [R, 4 k + 3]) -> {name: array} over PACKED_COLUMNS: sim as float32,
    valid as uint8, the rest int32."""
    width = sum(k if wide else 1 for _, wide in PACKED_COLUMNS)
    if packed.shape[1] != width:
        raise ValueError(f"{packed.shape[1]} packed columns, {width} expected at k = {k}")
    out, c0 = {}, 0
    for name, wide in PACKED_COLUMNS:
        out[name] = packed[:, c0:c0 + k] if wide else packed[:, c0]
        c0 += k if wide else 1
    out["sim"] = out["sim"].copy().view(np.float32)
    out["valid"] = out["valid"].astype(np.uint8)
    return out


def verifier_ok(n, inl, min_inliers, min_inlier_ratio):
    """The verifier's decision rule (geometric_verification.py:602-620) on host integers: the
    same float64 ratio and comparisons as pipeline.decide_pairs (tests/test_gate_plan_cpu.py)."""
    n, inl = np.asarray(n, np.int64), np.asarray(inl, np.int64)
    ratio = inl.astype(np.float64) / np.maximum(n, 1).astype(np.float64)
    return (n >= 5) & (inl >= min_inliers) & (ratio >= min_inlier_ratio)


class StreamPlan:
    """Host mirror of the streamed retrieval lists with one result slot per list entry.

    update() takes the rows an append changed; record() takes the verifier's results of the
    new pairs; counts() recomputes DeviceGate.step()'s dict from the live lists and the stored
    results.  An evicted entry's result is dropped: it can never return, because a row's list
    only gains better entries."""

    def __init__(self, capacity, k, strict_mode=True, verifier_floor_gating=True, verify=True, min_inliers=20,
                 min_inlier_ratio=0.25):
        self.capacity, self.k, self.n = int(capacity), int(k), 0
        self.limit = 0 if strict_mode else 1
        self.verifier_floor_gating, self.verify = bool(verifier_floor_gating), bool(verify)
        self.min_inliers, self.min_inlier_ratio = min_inliers, min_inlier_ratio
        c, kk = self.capacity, self.k
        self.idx = np.full((c, kk), -1, np.int32)
        self.sim = np.zeros((c, kk), np.float32)
        self.valid = np.zeros((c, kk), np.uint8)
        self.count = np.zeros(c, np.int32)
        # the result store, one slot per list entry: verified?, matches, inliers, geometric is_valid
        self.v_have = np.zeros((c, kk), bool)
        self.v_n = np.zeros((c, kk), np.int32)
        self.v_inl = np.zeros((c, kk), np.int32)
        self.v_ok = np.zeros((c, kk), bool)
        self.poses = {}  # (a, b) -> [4, 4] f64 of the live verified pairs that have one
        self.coder = FloorCoder()
        self.codes = np.zeros(c, np.int64)
        self.has = np.zeros(c, np.uint8)
        self.num = np.full(c, np.nan, np.float64)
        self.labelled = 0

    # ------------------------------------------------------------------ labels
    def add_labels(self, floor_labels):
        """The new keyframes' labels -> (codes int64, has uint8) for the device; also keeps the
        numeric labels of the gate's |floor_i - floor_j| > limit (None -> NaN, never rejects)."""
        lab = gate_plan.label_list(floor_labels)
        lo, hi = self.labelled, self.labelled + len(lab)
        if hi > self.capacity:
            raise ValueError(f"{hi} keyframes exceed the capacity {self.capacity}")
        codes, has = self.coder.extend(lab)
        self.codes[lo:hi], self.has[lo:hi] = codes, has
        self.num[lo:hi] = gate_plan.numeric_labels(lab)
        self.labelled = hi
        return codes, has

    # ------------------------------------------------------------------- lists
    @staticmethod
    def changed_rows(inserted, n_old, n_new):
        """The rows an append changed, ascending: old rows something entered, then the new rows."""
        return np.concatenate([np.nonzero(np.asarray(inserted) > 0)[0], np.arange(n_old, n_new)]).astype(np.int64)

    def _gate_rejects(self, a, b):
        return np.abs(self.num[a] - self.num[b]) > self.limit  # NaN compares False

    def update(self, n_new, rows, r_idx, r_sim, r_valid, r_count, r_nev, r_ev):
        """The changed rows' new lists (r_idx / r_sim / r_valid [R, k], r_count [R]) and, for the
        old ones among them, their evictions (r_nev [R], r_ev [R, k]; ignored for new rows).
        Returns a dict of (a, b) int32 array pairs: 'new' (every entry that entered a list),
        'verify' (those bound for the verifier: is_valid ones the floor skip lets through),
        'evicted', and 'retracted' (evicted pairs that had been accepted)."""
        n_old = self.n
        if not n_old < n_new <= self.labelled:
            raise ValueError(f"update to {n_new} keyframes from {n_old} with {self.labelled} labelled")
        new_a, new_b, new_valid, ev_a, ev_b, ev_acc = [], [], [], [], [], []
        for i, r in enumerate(np.asarray(rows).tolist()):
            c_new = int(r_count[i])
            ni = np.asarray(r_idx[i, :c_new], np.int32)
            is_new = np.ones(c_new, bool)
            if r < n_old:
                c_old, nev = int(self.count[r]), int(r_nev[i])
                keep = c_old - nev
                old = self.idx[r, :c_old].copy()
                is_new = ni >= n_old
                # a merge of two sorted lists: the stored entries that stay are a prefix, in order
                if not (np.array_equal(ni[~is_new], old[:keep]) and np.array_equal(r_ev[i, :nev], old[keep:])):
                    raise ValueError(f"row {r}: the update is not a merge of its stored list")
                acc = self.v_have[r, keep:c_old] & self.v_ok[r, keep:c_old] & ~self._gate_rejects(r, old[keep:])
                ev_a += [r] * nev
                ev_b += old[keep:].tolist()
                ev_acc += acc.tolist()
                for j in old[keep:].tolist():
                    self.poses.pop((r, j), None)
                for arr in (self.v_have, self.v_n, self.v_inl, self.v_ok):
                    kept = arr[r, :keep].copy()
                    arr[r] = 0
                    arr[r, :c_new][~is_new] = kept
            elif r >= n_new:
                raise ValueError(f"row {r} is past the {n_new} keyframes")
            self.idx[r, :c_new], self.sim[r, :c_new] = ni, r_sim[i, :c_new]
            self.valid[r, :c_new], self.count[r] = r_valid[i, :c_new], c_new
            new_a += [r] * int(is_new.sum())
            new_b += ni[is_new].tolist()
            new_valid += (np.asarray(r_valid[i, :c_new])[is_new] != 0).tolist()
        self.n = n_new
        arr = lambda x: np.asarray(x, np.int32)  # noqa: E731
        new_a, new_b, ev_a, ev_b = arr(new_a), arr(new_b), arr(ev_a), arr(ev_b)
        sel = np.asarray(new_valid, bool)
        va, vb = new_a[sel], new_b[sel]
        if self.verifier_floor_gating:
            same = gate_plan.same_floor(va, vb, self.codes, self.has)
            va, vb = va[same], vb[same]
        if not self.verify:
            va, vb = va[:0], vb[:0]
        acc = np.asarray(ev_acc, bool)
        return {"new": (new_a, new_b), "verify": (va, vb), "evicted": (ev_a, ev_b),
                "retracted": (ev_a[acc], ev_b[acc])}

    def _slots(self, pa, pb):
        hit = (self.idx[pa] == np.asarray(pb)[:, None]) & (np.arange(self.k)[None, :] < self.count[pa][:, None])
        if not hit.any(axis=1).all():
            raise ValueError("a recorded pair is not a live list entry")
        return hit.argmax(axis=1)

    def record(self, pa, pb, matches, inliers, pose=None):
        """Store the verifier's results of ordered pairs (pa, pb): match and inlier counts, and
        pose [P, 4, 4] when there is one.  Returns (ok, accepted): the geometric is_valid and
        whether the floor gate lets the pair through as well."""
        pa, pb = np.asarray(pa, np.int64), np.asarray(pb, np.int64)
        if len(pa) == 0:
            return np.zeros(0, bool), np.zeros(0, bool)
        s = self._slots(pa, pb)
        if self.v_have[pa, s].any():
            raise ValueError("an ordered pair was verified twice")
        ok = verifier_ok(matches, inliers, self.min_inliers, self.min_inlier_ratio)
        self.v_have[pa, s], self.v_n[pa, s], self.v_inl[pa, s], self.v_ok[pa, s] = True, matches, inliers, ok
        if pose is not None:
            for a, b, p in zip(pa.tolist(), pb.tolist(), np.asarray(pose, np.float64).reshape(-1, 4, 4)):
                self.poses[(a, b)] = p.copy()
        return ok, ok & ~self._gate_rejects(pa, pb)

    # ------------------------------------------------------------------ queries
    def _live(self):
        return np.arange(self.k)[None, :] < self.count[:self.n, None]

    def live_pairs(self):
        """Every ordered pair of the lists, row-major in emission order: (a, b) int32."""
        qs, js = np.nonzero(self._live())
        return qs.astype(np.int32), self.idx[qs, js]

    def _verified(self):
        """(qs, js) of the entries bound for the verifier, row-major; and the skipped count."""
        qs, js = np.nonzero(self._live() & (self.valid[:self.n] != 0))
        skipped = 0
        if self.verifier_floor_gating:
            same = gate_plan.same_floor(qs, self.idx[qs, js], self.codes, self.has)
            skipped = int((~same).sum())
            qs, js = qs[same], js[same]
        return qs, js, skipped

    def counts(self):
        """DeviceGate.step()'s dict on the keyframes seen so far, recomputed from the live
        lists and the result store."""
        n = self.n
        matches, floor_rej, _, _ = gate_plan.pairs_from_retrieval(self.idx[:n], self.valid[:n], self.count[:n], 0)
        out = dict.fromkeys(COUNT_KEYS, 0)
        out["matches"], out["retrieval_floor_rejected"] = matches, floor_rej
        if not self.verify:
            return out
        qs, js, out["skipped_floor_mismatch"] = self._verified()
        if not self.v_have[qs, js].all():
            raise ValueError("a live pair bound for the verifier has no result")
        ok = self.v_ok[qs, js]
        rej = ok & self._gate_rejects(qs, self.idx[qs, js])
        out["pairs_verified"], out["verified_valid"] = len(qs), int(ok.sum())
        out["verifier_invalid"] = len(qs) - int(ok.sum())
        out["gate_rejected_cross_floor"] = int(rej.sum())
        out["accepted"] = int(ok.sum()) - int(rej.sum())
        return out

    def pair_results(self):
        """The live verified pairs in gate_plan.pair_records' form, sorted by (a, b)."""
        qs, js, _ = self._verified() if self.verify else (np.zeros(0, np.int64),) * 2 + (0,)
        a, b = qs.astype(np.int32), self.idx[qs, js].astype(np.int32)
        o = np.lexsort((b, a))
        return {"a": a[o], "b": b[o], "matches": self.v_n[qs, js][o], "inliers": self.v_inl[qs, js][o],
                "is_valid": self.v_ok[qs, js][o]}

    def accepted_pairs(self):
        """The live pairs every stage accepts, row-major: (a, b) int32."""
        if not self.verify:
            return np.zeros(0, np.int32), np.zeros(0, np.int32)
        qs, js, _ = self._verified()
        b = self.idx[qs, js]
        acc = self.v_ok[qs, js] & ~self._gate_rejects(qs, b)
        return qs[acc].astype(np.int32), b[acc].astype(np.int32)
