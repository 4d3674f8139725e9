"""DeviceGate's host plan (mlgate.gate_plan) and its shared decision tail
(mlgate.pipeline.decide_pairs, held to its host form stream_plan.verifier_ok) on the CPU:
the pair list from the retrieval lists, the verifier's floor skip, the unordered-pair plan, chunk starts and bounds, the 'auto' chunk
arithmetic, LoFTR's frame-slot cache -- against the oracle chain's fixture
(tests/golden/gate_chain.npz, oracle.pipeline.gate_chain) and brute force.
"""
import json

import numpy as np
import pytest
import torch

from mlgate import gate_plan, stream_plan, synthetic
from mlgate.pipeline import decide_pairs
from mlgate.vpr import floor_codes
from oracle import pipeline as opipe

CFG = {"A": (True, True), "B": (False, True), "C": (False, False)}


@pytest.fixture(scope="module")
def chain(golden_dir):
    g = dict(np.load(f"{golden_dir}/gate_chain.npz"))
    n, places, seed, k = (int(x) for x in g["params"])
    plan = tuple((int(f), float(p)) for f, p in g["plan"])
    g["seq"] = synthetic.make_sequence(n, places, seed, plan)
    g["k"], (g["thr"], g["gap"]) = k, (float(x) for x in g["thr_gap"])
    g["counts"] = json.loads(str(g["counts"]))
    g["pair_index"] = {tuple(p): i for i, p in enumerate(g["pairs"].tolist())}
    return g


def retrieval_lists(q, m, valid, N, k):
    """The flat matches (emission order) as DeviceGate's [N, k] idx / valid and [N] count."""
    idx, val, count = np.zeros((N, k), np.int32), np.zeros((N, k), np.uint8), np.zeros(N, np.int32)
    for a, b, v in zip(q, m, valid):
        idx[a, count[a]], val[a, count[a]] = b, v
        count[a] += 1
    return idx, val, count


def chain_pairs(chain, cfg):
    """The plan's (pa, pb) of the fixture's configuration, before and after the floor skip."""
    N = len(chain["labels"])
    idx, val, count = retrieval_lists(chain[f"{cfg}_q"], chain[f"{cfg}_m"], chain[f"{cfg}_valid"], N, chain["k"])
    matches, floor_rej, pa, pb = gate_plan.pairs_from_retrieval(idx, val, count, 0)
    codes, has = floor_codes(chain["labels"].tolist())
    same = (gate_plan.same_floor(pa, pb, np.asarray(codes), np.asarray(has, np.uint8)) if CFG[cfg][1]
            else np.ones(len(pa), bool))
    return matches, floor_rej, pa, pb, same


@pytest.mark.parametrize("cfg", list(CFG))
def test_fixture_chain_through_the_plan_and_the_tail(chain, cfg):
    verdict = {tuple(p): {"is_valid": bool(v)} for p, v in zip(chain["pairs"].tolist(), chain["pair_valid"])}
    rg, vg = CFG[cfg]
    ref = opipe.gate_chain(chain["labels"], chain["desc"], chain["seq"].t, None, lambda a, b: verdict[(a, b)],
                           chain["gap"], chain["thr"], chain["k"], retrieval_gating=rg, verifier_gating=vg)
    for key in ("q", "m", "valid", "skip"):
        assert np.array_equal(ref[key], chain[f"{cfg}_{key}"]), key
    q, m, valid = ref["q"], ref["m"], ref["valid"]
    matches, floor_rej, pa, pb, same = chain_pairs(chain, cfg)
    assert pa.dtype == pb.dtype == np.int32
    assert matches == len(q) and floor_rej == ref["counts"]["retrieval_floor_rejected"]
    assert np.array_equal(pa, q[valid]) and np.array_equal(pb, m[valid])
    assert np.array_equal(~same, ref["skip"]) and int((~same).sum()) == ref["counts"]["skipped_floor_mismatch"]
    # the surviving pairs' fp32 match / inlier counts through the shared tail, in two chunks
    pa, pb = pa[same], pb[same]
    i = np.array([chain["pair_index"][(int(a), int(b))] for a, b in zip(pa, pb)], np.int64)
    f_num = torch.from_numpy(chain["labels"].astype(np.float64))
    n_valid_t, gate_rej_t = torch.zeros((), dtype=torch.int64), torch.zeros((), dtype=torch.int64)
    half = len(pa) // 2
    rec = []
    for sel in (np.arange(half), np.arange(half, len(pa))):
        n, inl = (torch.from_numpy(chain[key][i[sel]]) for key in ("pair_matches", "pair_inliers"))
        ok = decide_pairs(n, inl, torch.from_numpy(pa[sel]).long(), torch.from_numpy(pb[sel]).long(), f_num, 0,
                          20, 0.25, n_valid_t, gate_rej_t)
        # the host form of the rule (StreamingGate's) decides every pair as the device form does
        assert np.array_equal(stream_plan.verifier_ok(n.numpy(), inl.numpy(), 20, 0.25), ok.numpy())
        rec.append((sel, n.numpy(), inl.numpy(), ok.numpy()))
    r = gate_plan.pair_records(pa, pb, rec)
    assert np.array_equal(r["is_valid"], chain["pair_valid"][i])
    assert np.array_equal(r["matches"], chain["pair_matches"][i])
    assert np.array_equal(r["inliers"], chain["pair_inliers"][i])
    assert r["a"] is pa and r["b"] is pb and r["is_valid"].dtype == bool
    n_valid, gate_rej = int(n_valid_t), int(gate_rej_t)
    assert n_valid == int(r["is_valid"].sum()) and n_valid - gate_rej == int(chain[f"{cfg}_gate_valid"].sum())
    got = {"retrieval_floor_rejected": floor_rej, "skipped_floor_mismatch": int((~same).sum()),
           "verifier_invalid": len(pa) - n_valid, "gate_rejected_cross_floor": gate_rej}
    got["total"] = sum(got.values())
    assert got == ref["counts"] == chain["counts"][cfg]


def test_decision_rule_edges_device_form_equals_host_form():
    """(matches, inliers, min_inliers) -> is_valid at the rule's edges (geometric_verification.py:
    602-620: at least 5 matches, inliers >= min_inliers, inliers / matches >= 0.25), the same
    from decide_pairs on CPU tensors and from stream_plan.verifier_ok."""
    rows = [(0, 0, 0, False),      # no matches: the ratio's denominator is clamped, n < 5 decides
            (0, 0, 20, False),
            (4, 4, 0, False),      # every match an inlier, but fewer than 5 matches
            (5, 5, 5, True),       # the first n that can pass
            (5, 4, 5, False),
            (80, 20, 20, True),    # ratio exactly 0.25 passes
            (81, 20, 20, False),   # just under it
            (80, 19, 19, False)]
    f_num = torch.zeros(2, dtype=torch.float64)
    for n_, inl_, min_inl, want in rows:
        n, inl = torch.tensor([n_], dtype=torch.int32), torch.tensor([inl_], dtype=torch.int32)
        z = torch.zeros(1, dtype=torch.int64)
        n_valid_t, gate_rej_t = torch.zeros((), dtype=torch.int64), torch.zeros((), dtype=torch.int64)
        ok = decide_pairs(n, inl, z, z + 1, f_num, 0, min_inl, 0.25, n_valid_t, gate_rej_t)
        host = stream_plan.verifier_ok(np.array([n_], np.int32), np.array([inl_], np.int32), min_inl, 0.25)
        assert ok.tolist() == host.tolist() == [want], (n_, inl_, min_inl)
        assert int(n_valid_t) == int(want) and int(gate_rej_t) == 0
    # all rows at once, one min_inliers: the two forms agree element by element
    n = np.array([r[0] for r in rows], np.int32)
    inl = np.array([r[1] for r in rows], np.int32)
    z = torch.zeros(len(rows), dtype=torch.int64)
    ok = decide_pairs(torch.from_numpy(n), torch.from_numpy(inl), z, z, f_num, 0, 5, 0.25,
                      torch.zeros((), dtype=torch.int64), torch.zeros((), dtype=torch.int64))
    assert np.array_equal(ok.numpy(), stream_plan.verifier_ok(n, inl, 5, 0.25))


def test_pairs_from_retrieval_and_rerank_offsets():
    """Rows of a rank's shard are queries lo + row; entries past count are not pairs; the
    re-ranked lists replace the pair list in their own order."""
    idx = np.array([[7, 3, 9], [1, 2, 0], [5, 5, 5]], np.int32)
    val = np.array([[1, 0, 1], [0, 1, 1], [1, 1, 1]], np.uint8)
    matches, rej, pa, pb = gate_plan.pairs_from_retrieval(idx, val, np.array([3, 2, 0], np.int32), 10)
    assert (matches, rej) == (5, 2)
    assert pa.tolist() == [10, 10, 11] and pb.tolist() == [7, 9, 2] and pa.dtype == pb.dtype == np.int32
    ra, rb = gate_plan.pairs_from_rerank(np.array([[9, 7], [2, 0], [0, 0]], np.int32), np.array([2, 1, 0]), 10)
    assert ra.tolist() == [10, 10, 11] and rb.tolist() == [9, 7, 2] and ra.dtype == rb.dtype == np.int32
    e = gate_plan.pairs_from_retrieval(np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint8), np.zeros(0, np.int32), 0)
    assert e[:2] == (0, 0) and len(e[2]) == len(e[3]) == 0


def test_floor_skip_is_python_inequality():
    """Every ordered pair of distinct keyframes (a keyframe is never paired with itself:
    the time gap) against Python's floor1 != floor2."""
    lab = [1, 1.0, 2, None, float('nan'), float('nan'), np.int64(2), 'x', 'x']
    codes, has = floor_codes(lab)
    pa, pb = (x.ravel() for x in np.meshgrid(np.arange(len(lab)), np.arange(len(lab)), indexing="ij"))
    pa, pb = pa[pa != pb], pb[pa != pb]
    same = gate_plan.same_floor(pa, pb, np.asarray(codes), np.asarray(has, np.uint8))
    want = np.array([not (lab[a] != lab[b]) for a, b in zip(pa, pb)])
    assert np.array_equal(same, want)
    skipped = {(int(a), int(b)) for a, b in zip(pa[~same], pb[~same])}
    c2, h2 = floor_codes([None, None])  # None / None is not skipped
    assert gate_plan.same_floor(np.array([0]), np.array([1]), np.asarray(c2), np.asarray(h2, np.uint8)).all()
    assert (4, 5) in skipped and (5, 4) in skipped and (3, 0) in skipped and (0, 1) not in skipped
    assert (2, 6) not in skipped and (7, 8) not in skipped and (0, 7) in skipped


def random_pairs(seed, N=50, n=400):
    """Seeded ordered pairs with reversed duplicates (both orientations, and a > b alone)."""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, N, n), rng.integers(0, N, n)
    a, b = a[a != b], b[a != b]
    rev = rng.random(len(a)) < 0.4
    pa, pb = np.concatenate([a, b[rev]]), np.concatenate([b, a[rev]])
    _, first = np.unique(pa * N + pb, return_index=True)  # each ordered pair once, as retrieval emits them
    first.sort()
    return pa[first].astype(np.int32), pb[first].astype(np.int32), N


def check_unordered_plan(pa, pb, N):
    ua, ub, inv, swap, order = gate_plan.unordered_plan(pa, pb, N, True)
    assert np.array_equal(ua[inv], np.minimum(pa, pb)) and np.array_equal(ub[inv], np.maximum(pa, pb))
    assert np.array_equal(swap, (pa > pb)) and swap.dtype == np.uint8
    key = ua.astype(np.int64) * N + ub
    assert np.all(np.diff(key) > 0)  # strictly ascending: every unordered pair once
    assert ua.dtype == ub.dtype == np.int32
    assert np.array_equal(np.sort(order), np.arange(len(pa)))
    assert np.all(np.diff(inv[order]) >= 0)  # grouped by unordered pair ...
    same = np.diff(inv[order]) == 0
    assert np.all(np.diff(order)[same] > 0)  # ... and stable within a group
    return ua, ub, inv, swap, order


def test_unordered_plan(chain):
    _, _, pa, pb, _ = chain_pairs(chain, "C")
    ua, _, inv, swap, _ = check_unordered_plan(pa, pb, len(chain["labels"]))
    cnt = np.bincount(inv)  # the fixture has pairs in both orientations and pairs present as a > b alone
    assert int((cnt == 2).sum()) == 48 and int(((cnt[inv] == 1) & (swap == 1)).sum()) == 28
    assert len(ua) < len(pa) and set(swap.tolist()) == {0, 1}
    pa, pb, N = random_pairs(5)
    ua, _, inv, swap, _ = check_unordered_plan(pa, pb, N)
    assert len(ua) < len(pa) and set(swap.tolist()) == {0, 1}
    # dedup=False: the identity plan
    ia, ib, inv, swap, order = gate_plan.unordered_plan(pa, pb, N, False)
    assert ia is pa and ib is pb and not swap.any() and swap.dtype == np.uint8
    assert np.array_equal(inv, np.arange(len(pa))) and np.array_equal(order, np.arange(len(pa)))
    z = np.zeros(0, np.int32)
    for dedup in (True, False):
        assert [len(x) for x in gate_plan.unordered_plan(z, z, N, dedup)] == [0] * 5


@pytest.mark.parametrize("lg_tail", [0, 4])
@pytest.mark.parametrize("n", [0, 1, 2048, 2049, 3 * 2048 + 1500])
def test_chunk_starts_and_bounds(n, lg_tail):
    chunk = 2048
    # ordered pairs over n unordered ones: one or both orientations, grouped as `order` groups them
    inv_sorted = np.repeat(np.arange(n), 1 + (np.arange(n) % 3 == 0))
    starts, bounds = gate_plan.chunk_starts(n, chunk, lg_tail, inv_sorted)
    assert starts[0] == 0 and starts[-1] == n and np.all(np.diff(starts) > 0)
    sizes = np.diff(starts)
    assert np.all(sizes <= chunk)
    assert (len(sizes) == 0) == (n == 0)
    rem = n - (n - 1) // chunk * chunk if n else 0  # what the full chunks leave
    if lg_tail and rem >= 1024:
        assert sizes[-1] == max(256, rem // lg_tail) and len(sizes) == -(-n // chunk) + 1
    else:
        assert len(sizes) == -(-n // chunk)
    assert bounds[0] == 0 and bounds[-1] == len(inv_sorted) and len(bounds) == len(starts)
    for c in range(len(sizes)):  # every ordered pair in the chunk of its unordered index
        u = inv_sorted[bounds[c]:bounds[c + 1]]
        assert np.all((u >= starts[c]) & (u < starts[c + 1]))


def test_chunk_tail_floor_of_256():
    """rem // lg_tail below 256: the last chunk is 256."""
    starts, _ = gate_plan.chunk_starts(1024, 4096, 8, np.arange(1024))
    assert starts == [0, 768, 1024]


def test_auto_chunk():
    per = 3.5 * 2**20
    for n_pairs in (1, 255, 256, 257, 5000, 100000):
        for avail in (256 * per, 700 * per, 5119 * per, 6000 * per, 1e13):
            c = gate_plan.auto_chunk(avail, per, n_pairs)
            assert c % 256 == 0 and 256 <= c <= 5120 and c <= -(-n_pairs // 256) * 256
            assert c * per <= avail
            # the largest such chunk
            assert c == 5120 or c == -(-n_pairs // 256) * 256 or (c + 256) * per > avail
    for avail in (256 * per - 1, 0, -5.0):
        with pytest.raises(MemoryError):
            gate_plan.auto_chunk(avail, per, 1000)


@pytest.mark.parametrize("C, frames", [(4, 30), (48, 160)])
def test_slot_cache(C, frames):
    rng = np.random.default_rng(C)
    pa, pb = rng.integers(0, frames, 40 * C), rng.integers(0, frames, 40 * C)
    order = np.lexsort((pb, pa))
    cache = gate_plan.SlotCache(4 * C)
    evictions = held_hits = 0
    for c0 in range(0, len(order), C):
        sel = order[c0:c0 + C]
        frs = np.unique(np.concatenate([pa[sel], pb[sel]]))
        before, n_free = dict(cache.slot_of), len(cache.free)
        todo, slots = cache.assign(frs)
        evicted = [f for f in before if f not in cache.slot_of]
        if evicted:
            evictions += 1
            assert n_free < len(frs)  # only when the free rows do not cover the chunk
            assert set(evicted) == set(before) - set(frs.tolist())  # then every frame outside it
        else:
            assert not set(todo) & set(before)  # a held frame is not recomputed
        for f in before:
            if f in cache.slot_of:
                assert cache.slot_of[f] == before[f]  # nor moved
        held_hits += len(set(before) & set(frs.tolist()))
        assert len(todo) == len(slots) and [cache.slot_of[f] for f in todo] == slots
        assert set(frs.tolist()) <= set(cache.slot_of)
        assert set(todo) == set(frs.tolist()) - set(before)
        live = list(cache.slot_of.values())
        assert len(set(live)) == len(live) and all(0 <= s < 4 * C for s in live)
        assert sorted(live + cache.free) == list(range(4 * C))
    assert evictions > 0 and held_hits > 0
