"""mlgate.stream_plan on the CPU: the floor coder used incrementally against its one-shot use
(floor_codes), the packed changed-rows format's round trip, and a host replay of a streamed
sequence whose every prefix must give the plan exactly what gate_plan gives on that prefix's
full lists.  Every comparison is exact."""
import numpy as np
import pytest

from mlgate import gate_plan, stream_plan
from mlgate.vpr import floor_codes
from oracle import retrieval as oret

NAN = float("nan")


# ------------------------------------------------------------------ floor codes
LABELS = [3, 1, 1.0, NAN, None, "b", np.int64(3), np.float32(1.0), NAN, "b", None, 2.5, "a", np.float64("nan"), 0, 7]


@pytest.mark.parametrize("cut", range(len(LABELS) + 1))
def test_incremental_floor_codes_equal_floor_codes_on_the_concatenation(cut):
    want_codes, want_has = floor_codes(LABELS)
    coder = stream_plan.FloorCoder()
    c0, h0 = coder.extend(LABELS[:cut])
    c1, h1 = coder.extend(LABELS[cut:])
    assert np.array_equal(np.concatenate([c0, c1]), want_codes)
    assert np.array_equal(np.concatenate([h0, h1]), want_has)
    assert c0.dtype == np.int64 and h0.dtype == np.uint8


def test_incremental_floor_codes_one_label_at_a_time():
    want_codes, want_has = floor_codes(LABELS)
    coder = stream_plan.FloorCoder()
    parts = [coder.extend([f]) for f in LABELS]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), want_codes)
    assert np.array_equal(np.concatenate([p[1] for p in parts]), want_has)


# ------------------------------------------------------------ the packed transfer
@pytest.mark.parametrize("k", [1, 3, 32])
def test_packed_rows_round_trip(k):
    """Named arrays concatenated in PACKED_COLUMNS' order come back from unpack unchanged: sim
    bit for bit (NaN payloads, -0.0, infinities), negative idx / evicted entries, the widths
    at k = 1 (a wide column is still [R, 1])."""
    rng = np.random.default_rng(k)
    R = 9
    sim_bits = rng.integers(-2**31, 2**31, (R, k), dtype=np.int64).astype(np.int32)
    # quiet NaN, -0.0, NaNs with payloads (0xffffffff among them), 0.0, +inf, a denormal
    special = np.array([0x7fc00000, -2**31, 0x7fc00001, -1, 0, 0x7f800000, 1], np.int64).astype(np.int32)
    sim_bits.reshape(-1)[:len(special)] = special
    want = {"idx": rng.integers(-1, 5000, (R, k)).astype(np.int32), "sim": sim_bits,
            "valid": rng.integers(0, 2, (R, k)).astype(np.int32), "count": rng.integers(0, k + 1, R).astype(np.int32),
            "n_evicted": rng.integers(0, k + 1, R).astype(np.int32),
            "evicted": rng.integers(-1, 5000, (R, k)).astype(np.int32),
            "kp_count": rng.integers(0, 2049, R).astype(np.int32)}
    want["idx"][0], want["evicted"][-1] = -1, -1
    assert [name for name, _ in stream_plan.PACKED_COLUMNS] == list(want)
    packed = np.concatenate([want[name] if wide else want[name][:, None]
                             for name, wide in stream_plan.PACKED_COLUMNS], 1)
    assert packed.shape == (R, 4 * k + 3) and packed.dtype == np.int32
    got = stream_plan.unpack(packed, k)
    assert list(got) == list(want)
    for name, wide in stream_plan.PACKED_COLUMNS:
        assert got[name].shape == ((R, k) if wide else (R,)), name
    assert got["sim"].dtype == np.float32 and got["valid"].dtype == np.uint8
    assert np.array_equal(got["sim"].view(np.int32), want["sim"])
    for name in want:
        if name != "sim":
            assert np.array_equal(got[name], want[name]), name
    assert np.isnan(got["sim"]).any() and np.signbit(got["sim"][got["sim"] == 0]).any()
    with pytest.raises(ValueError):
        stream_plan.unpack(packed[:, :-1], k)


# ----------------------------------------------------------------------- replay
N, D, K, GAP, THR = 120, 16, 5, 10.0, 0.25
MIN_INL, MIN_RATIO = 20, 0.25


def before(va, ia, vb, ib):
    return va > vb or (va == vb and ia > ib)


def sort_rule(entries):
    """(sim, idx) entries in the order (sim desc, index desc)."""
    return sorted(entries, key=lambda e: (-e[0], -e[1]))


@pytest.fixture(scope="module")
def seq():
    rng = np.random.default_rng(5)
    desc = rng.standard_normal((N, D)).astype(np.float32)
    for i in range(3, N, 3):                      # many duplicated rows: exact ties
        desc[i] = desc[rng.integers(0, i)]
    t = 50.0 + 0.765 * np.arange(N)
    pool = [0, 1, 1.0, 2, None, NAN]
    labels = [pool[i] for i in rng.integers(0, len(pool), N)]
    S = oret.pairwise_similarities(desc)
    chunks = []
    while sum(chunks) < N:
        chunks.append(min(int(rng.integers(1, 17)), N - sum(chunks)))
    return {"desc": desc, "t": t, "labels": labels, "S": S, "chunks": chunks}


def survivors(S, t, i, cols):
    return [(S[i, j], j) for j in cols if not abs(t[j] - t[i]) < GAP and not S[i, j] < np.float32(THR)]


def replay_append(S, t, codes, has, gating, lists, n_old, n_new):
    """One append under the stated rule with plain Python: (inserted, evictions per old row);
    `lists` (row -> [(sim, idx, valid)]) is updated in place."""
    def bit(i, j):
        return 0 if gating and has[i] and has[j] and codes[i] != codes[j] else 1
    inserted, evicted = np.zeros(n_old, np.int32), {}
    for i in range(n_old):
        old = [(s, j) for s, j, _ in lists[i]]
        merged = sort_rule(old + survivors(S, t, i, range(n_old, n_new)))[:K]
        inserted[i] = sum(1 for e in merged if e[1] >= n_old)
        evicted[i] = [j for _, j in old if (_, j) not in merged] if inserted[i] else []
        lists[i] = [(s, j, bit(i, j)) for s, j in merged]
    for i in range(n_old, n_new):
        lists[i] = [(s, j, bit(i, j)) for s, j in sort_rule(survivors(S, t, i, range(n_new)))[:K]]
    return inserted, evicted


def dense(lists, n):
    idx, sim = np.full((n, K), -1, np.int32), np.zeros((n, K), np.float32)
    valid, count = np.zeros((n, K), np.uint8), np.zeros(n, np.int32)
    for i in range(n):
        for s, (v, j, b) in enumerate(lists[i]):
            idx[i, s], sim[i, s], valid[i, s] = j, v, b
        count[i] = len(lists[i])
    return idx, sim, valid, count


def fake_verifier(pa, pb):
    """A deterministic (matches, inliers) per ordered pair, covering every branch of the rule."""
    pa, pb = np.asarray(pa, np.int64), np.asarray(pb, np.int64)
    n = (pa * 7 + pb * 13) % 90
    return n.astype(np.int32), ((pa * 3 + pb * 5) % (n + 1)).astype(np.int32)


def batch_counts(idx, valid, count, codes, has, num, vfg, limit):
    """DeviceGate.step()'s counts from a prefix's full lists, with gate_plan's own functions."""
    matches, floor_rej, pa, pb = gate_plan.pairs_from_retrieval(idx, valid, count, 0)
    out = {"matches": matches, "retrieval_floor_rejected": floor_rej, "skipped_floor_mismatch": 0}
    if vfg:
        same = gate_plan.same_floor(pa, pb, codes, has)
        out["skipped_floor_mismatch"] = int((~same).sum())
        pa, pb = pa[same], pb[same]
    n, inl = fake_verifier(pa, pb)
    ok = (n >= 5) & (inl >= MIN_INL) & (inl.astype(np.float64) / np.maximum(n, 1) >= MIN_RATIO)
    rej = ok & (np.abs(num[pa] - num[pb]) > limit)
    out.update(pairs_verified=len(pa), verified_valid=int(ok.sum()), verifier_invalid=int((~ok).sum()),
               gate_rejected_cross_floor=int(rej.sum()), accepted=int(ok.sum() - rej.sum()))
    return out, pa, pb, ok & ~rej


@pytest.mark.parametrize("gating,vfg,strict", [(True, True, True), (False, True, False), (False, False, True)])
def test_replay_equals_the_batch_plan_on_every_prefix(seq, gating, vfg, strict):
    S, t, labels = seq["S"], seq["t"], seq["labels"]
    codes_all, has_all = floor_codes(labels)
    num = np.array([np.nan if v is None else float(v) for v in labels])
    plan = stream_plan.StreamPlan(N, K, strict_mode=strict, verifier_floor_gating=vfg, min_inliers=MIN_INL,
                                  min_inlier_ratio=MIN_RATIO)
    lists, n_old = {}, 0
    ever_verified, closures, saw_eviction, saw_retraction = set(), set(), False, False
    for c in seq["chunks"]:
        n_new = n_old + c
        codes, has = plan.add_labels(labels[n_old:n_new])
        assert np.array_equal(codes, codes_all[n_old:n_new]) and np.array_equal(has, has_all[n_old:n_new])
        prev = {i: [j for _, j, _ in lists[i]] for i in range(n_old)}
        inserted, evicted = replay_append(S, t, codes_all, has_all, gating, lists, n_old, n_new)
        idx, sim, valid, count = dense(lists, n_new)

        # the replay itself is the reference's retrieval on the prefix
        q, m, rs, rv = oret.find_loop_closures(seq["desc"][:n_new], t[:n_new], codes_all[:n_new], has_all[:n_new],
                                               GAP, THR, K, gating, S=np.ascontiguousarray(S[:n_new, :n_new]))
        live = np.arange(K)[None, :] < count[:, None]
        assert np.array_equal(np.repeat(np.arange(n_new), count), q) and np.array_equal(idx[live], m)
        assert np.array_equal(sim[live].view(np.int32), rs.view(np.int32)) and np.array_equal(valid[live], rv)

        rows = plan.changed_rows(inserted, n_old, n_new)
        r_ev = np.full((len(rows), K), -1, np.int32)
        r_nev = np.zeros(len(rows), np.int32)
        for i, r in enumerate(rows):
            if r < n_old:
                r_nev[i] = len(evicted[r])
                r_ev[i, :r_nev[i]] = evicted[r]
        up = plan.update(n_new, rows, idx[rows], sim[rows], valid[rows], count[rows], r_nev, r_ev)

        # new pairs and evictions: the set difference of the lists before and after
        now = {i: list(idx[i, :count[i]]) for i in range(n_new)}
        want_new = [(i, j) for i in range(n_new) for j in now[i] if j not in prev.get(i, [])]
        want_ev = [(i, j) for i in range(n_old) for j in prev[i] if j not in now[i]]
        assert list(zip(*(x.tolist() for x in up["new"]))) == want_new
        assert list(zip(*(x.tolist() for x in up["evicted"]))) == want_ev
        saw_eviction |= bool(want_ev)
        assert {(a, b) for a, b in zip(*(x.tolist() for x in up["retracted"]))} == closures & set(want_ev)
        saw_retraction |= len(up["retracted"][0]) > 0
        closures -= set(want_ev)

        # the pairs bound for the verifier: the new ones among the batch plan's
        want, bpa, bpb, bacc = batch_counts(idx, valid, count, codes_all, has_all, num, vfg, 0 if strict else 1)
        bound = set(zip(bpa.tolist(), bpb.tolist()))
        va, vb = up["verify"]
        assert list(zip(va.tolist(), vb.tolist())) == [p for p in want_new if p in bound]
        assert not (set(zip(va.tolist(), vb.tolist())) & ever_verified)        # never twice
        ever_verified |= set(zip(va.tolist(), vb.tolist()))
        # the canonical orientation (StreamingGate's plan: unordered_plan over the keyframes
        # seen) is the batch's (min, max)
        ua, ub, inv, swap, _ = gate_plan.unordered_plan(va, vb, max(plan.n, 1))
        assert np.array_equal(ua[inv], np.minimum(va, vb)) and np.array_equal(ub[inv], np.maximum(va, vb))
        assert np.array_equal(swap, (va > vb).astype(np.uint8))

        n_m, n_i = fake_verifier(va, vb)
        _, acc = plan.record(va, vb, n_m, n_i)
        closures |= {(int(a), int(b)) for a, b in zip(va[acc], vb[acc])}

        # live pairs, counts, accepted set and records: the batch's on this prefix
        la, lb = plan.live_pairs()
        assert np.array_equal(la, np.repeat(np.arange(n_new), count)) and np.array_equal(lb, idx[live])
        assert plan.counts() == want
        assert list(plan.counts()) == list(stream_plan.COUNT_KEYS)
        aa, ab = plan.accepted_pairs()
        assert set(zip(aa.tolist(), ab.tolist())) == set(zip(bpa[bacc].tolist(), bpb[bacc].tolist())) == closures
        pr = plan.pair_results()
        o = np.lexsort((bpb, bpa))
        bn, bi = fake_verifier(bpa[o], bpb[o])
        assert np.array_equal(pr["a"], bpa[o]) and np.array_equal(pr["b"], bpb[o])
        assert np.array_equal(pr["matches"], bn) and np.array_equal(pr["inliers"], bi)
        n_old = n_new
    assert saw_eviction and saw_retraction and plan.counts()["accepted"] > 0


def test_plan_refuses_a_pair_verified_twice_and_an_unknown_pair():
    plan = stream_plan.StreamPlan(4, 2, verifier_floor_gating=False)
    plan.add_labels([1, 1, 1])
    idx = np.array([[2, -1], [2, -1], [0, 1]], np.int32)
    up = plan.update(3, np.arange(3), idx, np.ones((3, 2), np.float32), np.ones((3, 2), np.uint8),
                     np.array([1, 1, 2], np.int32), np.zeros(3, np.int32), np.full((3, 2), -1, np.int32))
    assert list(zip(*(x.tolist() for x in up["verify"]))) == [(0, 2), (1, 2), (2, 0), (2, 1)]
    with pytest.raises(ValueError):
        plan.counts()                            # bound for the verifier, no result yet
    plan.record(*up["verify"], [30] * 4, [25] * 4)
    assert plan.counts()["accepted"] == 4
    with pytest.raises(ValueError):
        plan.record([0], [2], [30], [25])
    with pytest.raises(ValueError):
        plan.record([0], [1], [30], [25])
    with pytest.raises(ValueError):
        plan.add_labels([1, 1])
