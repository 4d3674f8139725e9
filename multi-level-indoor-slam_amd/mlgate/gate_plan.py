"""DeviceGate's host plan: how floor labels are coded, which pairs exist, which are skipped,
how they are grouped, chunked and recorded.  numpy only -- no device, no native library -- so
every decision here is checked on the CPU (tests/test_gate_plan_cpu.py); mlgate.pipeline and
mlgate.lg_pairs run the device work these plans drive.  (csrc/pair_plan.h is the same split
for the matchers' C++ side.)
"""
import numpy as np


def _row_major(idx, keep, lo):
    """(pa, pb) int32 of the kept entries of a [Q, k] list, row-major by query."""
    qs, js = np.nonzero(keep)
    return (qs + lo).astype(np.int32), idx[qs, js].astype(np.int32)


def pairs_from_retrieval(h_idx, h_valid, h_count, lo):
    """The retrieval lists of query rows [lo, lo + Q) (idx / valid [Q, k], count [Q]) ->
    (matches, retrieval_floor_rejected, pa, pb): the emitted matches, those with
    PlaceMatch.is_valid == False (emitted but floor-rejected), and the is_valid ones as
    the pairs handed to verify_with_semantics, row-major by query."""
    live = np.arange(h_idx.shape[1])[None, :] < h_count[:, None]
    pa, pb = _row_major(h_idx, live & (h_valid != 0), lo)
    return int(h_count.sum()), int((live & (h_valid == 0)).sum()), pa, pb


def pairs_from_rerank(r_idx, r_count, lo):
    """The re-ranked lists (r_idx [Q, top_k], r_count [Q]) -> (pa, pb): the kept entries,
    in re-ranked order within a row."""
    return _row_major(r_idx, np.arange(r_idx.shape[1])[None, :] < r_count[:, None], lo)


def pairs_from_sequence(h_idx, h_keep, lo):
    """The retrieval lists after the sequence-consistency check (idx / keep [Q, k]; keep is 0
    for every entry that was no candidate) -> (pa, pb): the kept entries, row-major by query
    in emission order."""
    return _row_major(h_idx, h_keep != 0, lo)


class FloorCoder:
    """Integer codes with the reference's equality semantics for the floor check
    ``query_floor == match_floor`` (place_recognition.py:896-899): labels that compare
    equal in Python share a code (1 and 1.0 included), every NaN gets its own code
    (NaN != NaN), None marks "no label" (has = 0).  One coder across several extend() calls
    gives the codes of one call on the concatenation (StreamingGate's appends)."""

    def __init__(self):
        self.seen, self.nxt = {}, 0

    def extend(self, labels):
        """(codes int64, has uint8) of the new labels."""
        codes = np.zeros(len(labels), np.int64)
        has = np.ones(len(labels), np.uint8)
        for i, f in enumerate(labels):
            if f is None:
                has[i] = 0
            elif isinstance(f, (float, np.floating)) and f != f:
                codes[i] = self.nxt
                self.nxt += 1
            else:
                key = f.item() if isinstance(f, np.generic) else f
                if key not in self.seen:
                    self.seen[key] = self.nxt
                    self.nxt += 1
                codes[i] = self.seen[key]
        return codes, has


def floor_codes(labels):
    """(codes int64, has uint8) of a whole list of labels: FloorCoder's rule."""
    return FloorCoder().extend(labels)


def label_list(floor_labels):
    """The labels as Python objects (an object array keeps its elements; any other array
    goes through tolist)."""
    lab = np.asarray(floor_labels)
    return list(lab) if lab.dtype == object else list(lab.tolist())


def numeric_labels(lab):
    """label_list's labels as the float64 array of the gate's |floor_i - floor_j| > limit
    (loop_closure_gate.py:91-98): None is NaN, which never rejects."""
    return np.array([np.nan if v is None else float(v) for v in lab], np.float64)


def same_floor(pa, pb, h_codes, h_has):
    """The pairs verify_with_semantics does NOT skip: it skips when floor1 != floor2 in
    Python (geometric_verification.py:709-710) -- None == None only, NaN != NaN (equality
    codes of floor_codes: every NaN keyframe has its own code)."""
    ha, hb = h_has[pa] != 0, h_has[pb] != 0
    return (ha & hb & (h_codes[pa] == h_codes[pb])) | (~ha & ~hb)


def unordered_plan(pa, pb, N, dedup=True):
    """(ua, ub, inv, swap, order) for matching each unordered pair once: the distinct
    (min, max) pairs in ascending key order, inv[i] = the unordered pair of ordered pair i,
    swap[i] = 1 where pair i is the (max, min) orientation, order = the ordered pairs
    grouped by unordered pair (stable).  dedup=False: every ordered pair is its own."""
    if dedup:
        key = np.minimum(pa, pb).astype(np.int64) * N + np.maximum(pa, pb)
        ukey, inv = np.unique(key, return_inverse=True)
        ua, ub = (ukey // N).astype(np.int32), (ukey % N).astype(np.int32)
        swap = (pa > pb).astype(np.uint8)
    else:
        ua, ub, inv, swap = pa, pb, np.arange(len(pa)), np.zeros(len(pa), np.uint8)
    return ua, ub, inv, swap, np.argsort(inv, kind="stable")


def chunk_starts(n_unordered, chunk, lg_tail, inv_sorted):
    """(starts, bounds): chunk c matches unordered pairs [starts[c], starts[c + 1]) and
    decides the ordered pairs order[bounds[c]:bounds[c + 1]] (inv_sorted = inv[order]).
    Full chunks, then (lg_tail > 0) the remainder cut so the LAST chunk is 1 / lg_tail of
    it -- that chunk's RANSAC is the only one with no LightGlue to overlap (per-pair
    results do not depend on the chunking)."""
    starts = list(range(0, n_unordered, chunk))
    rem = n_unordered - starts[-1] if starts else 0
    if lg_tail > 0 and rem >= 1024:
        starts.append(n_unordered - max(256, rem // lg_tail))
    starts.append(n_unordered)
    return starts, np.searchsorted(inv_sorted, np.asarray(starts))


def auto_chunk(avail_bytes, per_pair_bytes, n_pairs):
    """Pairs per LightGlue call for lg_chunk='auto': the largest multiple of 256 (<= 5120,
    bench.py's measured optimum, and no more than the pairs need) whose workspaces fit in
    avail_bytes."""
    chunk = int(max(avail_bytes, 0) // per_pair_bytes) // 256 * 256
    if chunk < 256:
        raise MemoryError(f"LightGlue needs {per_pair_bytes * 256 / 2**30:.1f} GiB for 256 pairs; "
                          f"{max(avail_bytes, 0) / 2**30:.1f} GiB free")
    return min(chunk, 5120, max(256, -(-n_pairs // 256) * 256))


class SlotCache:
    """Which row of a `capacity`-row feature buffer holds which keyframe, across the chunks
    of a (query, match)-ordered pair list.  A chunk of C pairs names at most 2 C keyframes;
    with capacity 4 C the previous chunk's stay held beside them."""

    def __init__(self, capacity):
        self.slot_of, self.free = {}, list(range(capacity))

    def assign(self, frs):
        """frs: the chunk's distinct keyframes -> (todo, slots): those not held, whose
        features the caller computes, and the rows they go to.  Every frame of frs has its
        slot_of entry afterwards.  Only when the free rows do not cover frs is every
        keyframe outside the chunk evicted."""
        if len(self.free) < len(frs):
            keep = set(int(f) for f in frs)
            for f in [f for f in self.slot_of if f not in keep]:
                self.free.append(self.slot_of.pop(f))
        todo = [int(f) for f in frs if int(f) not in self.slot_of]
        slots = [self.free.pop() for _ in todo]
        self.slot_of.update(zip(todo, slots))
        return todo, slots


def pair_records(pa, pb, rec):
    """last_pair_results: every verified ordered pair's (a, b, matches, inliers, is_valid)
    in verification order, from the chunks' (sel, n, inl, ok) host arrays."""
    r = {"a": pa, "b": pb, "matches": np.zeros(len(pa), np.int32), "inliers": np.zeros(len(pa), np.int32),
         "is_valid": np.zeros(len(pa), bool)}
    for sel, n, inl, ok in rec:
        r["matches"][sel], r["inliers"][sel], r["is_valid"][sel] = n, inl, ok
    return r
