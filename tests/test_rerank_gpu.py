"""mlg_rerank_gate on the GPU: the fused cross-correlation kernel against mlg_xcorr_batch bit
for bit, the selection kernel against the float64 restatement (tests/rerank_restatement.py)
exactly, the reference's recorded output, and the stage inside both composed gates."""
import os

import numpy as np
import pytest
import torch

from mlgate import _native, retrieval
from rerank_restatement import crafted_lists, rerank_rows

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _xb(feats_d, qa, qb):
    """mlg_xcorr_batch scores (host float32) of the pairs (qa[p], qb[p]) on the device bank."""
    dev = feats_d.device
    return _native.ops().xcorr_batch(feats_d, _t(np.asarray(qa, np.int32), dev),
                                     _t(np.asarray(qb, np.int32), dev)).cpu().numpy()


def _run(feats_d, idx, sim, mask, count, top_k, q0=0, cached=None, totals=True):
    dev = feats_d.device
    tot = torch.zeros(1, dtype=torch.int64, device=dev) if totals else None
    out = retrieval.rerank_gate(feats_d, _t(idx, dev), _t(sim, dev), _t(mask, dev), _t(count, dev), top_k, q0=q0,
                                cached=_t(cached, dev), totals=tot)
    return tuple(x.cpu().numpy() for x in out) + (int(tot.item()) if totals else None,)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want):
    """Every output of the op equals the restatement's: indices, order, global similarity and
    cross score bits (NaN where not scored), the float64 combined score, counts, dropped."""
    names = ("r_idx", "r_sim", "r_cross", "r_score", "r_count")
    for n, g, w in zip(names, got, want):
        if n == "r_cross":
            assert np.array_equal(np.isnan(g), np.isnan(w)), n
            assert np.array_equal(_bits(g)[~np.isnan(g)], _bits(w.astype(np.float32))[~np.isnan(w)]), n
        elif n in ("r_sim", "r_score"):
            assert g.dtype == w.dtype and np.array_equal(_bits(g), _bits(w)), n
        else:
            assert np.array_equal(g, w), n
    assert got[5] == want[5], "dropped total"


def _table_cross(feats_d, pairs):
    """{(a, b): mlg_xcorr_batch score} for the restatement's cross(a, b)."""
    pairs = sorted(set(pairs))
    if not pairs:
        return lambda a, b: (_ for _ in ()).throw(KeyError((a, b)))
    sc = _xb(feats_d, [a for a, _ in pairs], [b for _, b in pairs])
    table = {p: s for p, s in zip(pairs, sc)}
    return lambda a, b: table[(a, b)]


def _all_pairs(F, q0, Q):
    return [(a, b) for a in range(q0, q0 + Q) for b in range(F)]


def _golden_feats():
    return np.load(os.path.join(GOLD, "xcorr.npz"))["feats"].astype(np.float32)[:, 0]


# the golden's 6 frames (L = 528: four full tiles and a ragged fifth of 16); a ragged tile of
# 15 that is no multiple of 4; a single partial tile
@pytest.mark.parametrize("shape", ["golden", (9, 143, 384), (5, 35, 64)], ids=str)
def test_cross_is_xcorr_batch_bit_for_bit_in_both_orders(dev, shape):
    """Every ordered pair of the bank in the lists, top_k = k so that every entry is kept:
    r_cross of (i, j) has mlg_xcorr_batch's bits for (i, j) and for (j, i)."""
    if shape == "golden":
        feats = _golden_feats()
    else:
        feats = np.random.default_rng(shape[1]).standard_normal(shape).astype(np.float32)
    F = len(feats)
    fd = _t(feats, dev)
    idx = np.tile(np.arange(F, dtype=np.int32), (F, 1))
    sim = np.random.default_rng(1).uniform(0.2, 0.9, (F, F)).astype(np.float32)
    count = np.full(F, F, np.int32)
    r_idx, r_sim, r_cross, r_score, r_count, dropped = _run(fd, idx, sim, None, count, F)
    assert np.all(r_count == F) and dropped == 0
    qa, qb = np.repeat(np.arange(F), F), np.tile(np.arange(F), F)
    fwd = _xb(fd, qa, qb).reshape(F, F)
    rev = _xb(fd, qb, qa).reshape(F, F)
    got = np.full((F, F), np.nan, np.float32)
    for i in range(F):
        assert sorted(r_idx[i].tolist()) == list(range(F))
        got[i, r_idx[i]] = r_cross[i]
    assert np.array_equal(_bits(got), _bits(fwd))
    assert np.array_equal(_bits(got), _bits(rev))
    _same((r_idx, r_sim, r_cross, r_score, r_count, dropped),
          rerank_rows(idx, sim, None, count, lambda a, b: fwd[a, b], F, F=F))


@pytest.mark.parametrize("top_k", [1, 3, 6])
@pytest.mark.parametrize("use_mask,use_cached", [(True, True), (False, True), (True, False), (False, False)])
def test_selection_equals_the_restatement(dev, top_k, use_mask, use_cached):
    """Crafted lists: an exact tie (identical frames, equal sim), interleaved unmasked entries,
    uncached frames (a query among them), out-of-range indices, count 0 / below top_k / past k,
    q0 = 1."""
    feats, idx, sim, mask, count, q0, cached = crafted_lists(7, L=35, D=64)
    idx[4, 1], idx[4, 2] = 9, -3  # outside [0, F): not cached, never read
    mask[4, 1:3] = 1
    m, c = (mask if use_mask else None), (cached if use_cached else None)
    fd = _t(feats, dev)
    cross = _table_cross(fd, _all_pairs(len(feats), q0, len(count)))
    want = rerank_rows(idx, sim, m, count, cross, top_k, q0=q0, cached=c, F=len(feats))
    _same(_run(fd, idx, sim, m, count, top_k, q0=q0, cached=c), want)
    if top_k == 6 and use_mask and use_cached:
        row = want[0][0].tolist()  # the tie keeps emission order: frame 2 right before frame 5
        assert row.index(2) + 1 == row.index(5)
        assert want[3][0][row.index(2)] == want[3][0][row.index(5)]


def test_golden_rerank(dev):
    """CricaVPR.rerank_candidates' own output (tests/golden/xcorr.npz): rr for the cached
    query 0 (candidate 5 not cached: its score is the global one), rr_nocache for query 5."""
    g = dict(np.load(os.path.join(GOLD, "xcorr.npz")))
    fd = _t(_golden_feats(), dev)
    cands = g["cands"]
    idx = np.tile(cands[:, 0].astype(np.int32), (6, 1))
    sim = np.tile(cands[:, 1].astype(np.float32), (6, 1))
    count = np.full(6, len(cands), np.int32)
    cached = np.array([1, 1, 1, 1, 1, 0], np.uint8)
    r_idx, _, r_cross, r_score, r_count, _ = _run(fd, idx, sim, None, count, 4, cached=cached)
    assert np.array_equal(r_idx[0], g["rr"][:, 0].astype(np.int32)) and r_count[0] == 4
    assert np.max(np.abs(r_score[0] - g["rr"][:, 1])) < 1e-5  # test_xcorr_golden's tolerance
    assert np.isnan(r_cross[0][r_idx[0] == 5]).all()
    r_idx, _, r_cross, r_score, r_count, _ = _run(fd, idx, sim, None, count, 3, cached=cached)
    assert np.array_equal(r_idx[5], g["rr_nocache"][:, 0].astype(np.int32)) and r_count[5] == 3
    assert np.max(np.abs(r_score[5] - g["rr_nocache"][:, 1])) < 1e-5 and np.isnan(r_cross[5]).all()


def test_more_rows_and_pairs_than_are_resident(dev):
    """Q = 600, k = 8 at L = 35: 21,000 rows to normalise and 4,800 candidate slots, more than
    the device holds at once; against mlg_xcorr_batch and the restatement, and a repeated call
    is bit-identical."""
    rng = np.random.default_rng(11)
    F, L, D, Q, k, q0 = 640, 35, 64, 600, 8, 17
    feats = rng.standard_normal((F, L, D)).astype(np.float32)
    idx = rng.integers(0, F, (Q, k)).astype(np.int32)
    sim = rng.uniform(0.2, 0.9, (Q, k)).astype(np.float32)
    count = rng.integers(0, k + 1, Q).astype(np.int32)
    mask = (rng.random((Q, k)) > 0.25).astype(np.uint8)
    fd = _t(feats, dev)
    cross = _table_cross(fd, [(q0 + i, int(idx[i, s])) for i in range(Q) for s in range(k)])
    got = _run(fd, idx, sim, mask, count, 3, q0=q0)
    _same(got, rerank_rows(idx, sim, mask, count, cross, 3, q0=q0, F=F))
    again = _run(fd, idx, sim, mask, count, 3, q0=q0)
    for a, b in zip(got[:5], again[:5]):
        assert np.array_equal(_bits(a), _bits(b))
    assert got[5] == again[5] > 0


def test_python_refusals(dev):
    fd = torch.zeros(4, 35, 64, device=dev)
    idx, sim = torch.zeros(2, 3, dtype=torch.int32, device=dev), torch.zeros(2, 3, device=dev)
    count = torch.zeros(2, dtype=torch.int32, device=dev)
    for top_k in (0, 4):
        with pytest.raises(ValueError):
            retrieval.rerank_gate(fd, idx, sim, None, count, top_k)
    wide = torch.zeros(2, 65, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        retrieval.rerank_gate(fd, wide, torch.zeros(2, 65, device=dev), None, count, 2)
    with pytest.raises(RuntimeError):
        retrieval.rerank_gate(fd, idx, sim, None, count, 2, q0=3)  # q0 + Q > F


# ------------------------------------------------------------- inside the gates
GATE_K, GATE_TOP = 5, 2


@pytest.fixture(scope="module")
def gates(dev):
    """The 40-keyframe synthetic fixture sequence through DeviceGate with re-ranking off, with
    rerank_top_k = 2 and with rerank_top_k = k; threshold -1 and no retrieval floor gate, so
    every row emits k valid entries."""
    from mlgate import synthetic
    from mlgate.pipeline import DeviceGate
    from oracle import geometry as ogeo
    g = np.load(os.path.join(GOLD, "gate_chain.npz"))
    n, places, seed, _ = (int(x) for x in g["params"])
    seq = synthetic.make_sequence(n, places, seed, tuple((int(f), float(p)) for f, p in g["plan"]))
    labels = np.asarray(g["labels"])
    frames = torch.from_numpy(synthetic.frames_host(seq)).to(dev)
    kw = dict(device=str(dev), k=GATE_K, similarity_threshold=-1.0, min_time_gap=float(g["thr_gap"][1]),
              retrieval_floor_gating=False, K=ogeo.ISEC_K, vit_batch=64, lg_chunk=64, record=True)
    out = {"seq": seq, "labels": labels, "frames": frames, "kw": kw}
    for name, top in (("off", None), ("on", GATE_TOP), ("all", GATE_K + 3)):
        gate = DeviceGate(frames, seq.t, labels, rerank_top_k=top, **kw)
        out[name] = (gate, gate.step())
    return out


def _pair_rows(gate):
    r = gate.last_pair_results
    return {(int(a), int(b)): (int(n), int(i), bool(v))
            for a, b, n, i, v in zip(r["a"], r["b"], r["matches"], r["inliers"], r["is_valid"])}


def test_device_gate_reranks_between_retrieval_and_verification(dev, gates):
    g_off, o_off = gates["off"]
    g_on, o_on = gates["on"]
    h_idx, h_sim, h_valid, h_count = g_off.last_retrieval
    live = np.arange(GATE_K)[None, :] < h_count[:, None]
    nvalid = (live & (h_valid != 0)).sum(1)
    assert (nvalid > GATE_TOP).any()  # the stage has something to drop
    assert g_off.last_rerank is None and "reranked_out" not in o_off and "rerank_candidates" not in o_off
    # the retrieval lists are unchanged
    for a, b in zip(g_off.last_retrieval, g_on.last_retrieval):
        assert a.dtype == b.dtype and np.array_equal(_bits(a) if a.dtype.kind == "f" else a,
                                                     _bits(b) if b.dtype.kind == "f" else b)
    # the kept set is the restatement's, fed with mlg_xcorr_batch scores of the gate's own bank
    cross = _table_cross(g_on.local_feats, [(i, int(h_idx[i, s])) for i in range(len(h_count))
                                            for s in range(int(h_count[i]))])
    want = rerank_rows(h_idx, h_sim, h_valid, h_count, cross, GATE_TOP, F=g_on.N)
    r_idx, r_sim, r_cross, r_score, r_count = g_on.last_rerank
    _same((r_idx, r_sim, r_cross, r_score, r_count, want[5]), want)
    kept = [(i, int(j)) for i in range(len(r_count)) for j in r_idx[i, :r_count[i]]]
    # counts add up
    assert o_on["rerank_candidates"] == int(nvalid.sum())
    assert o_on["reranked_out"] == int(nvalid.sum()) - len(kept) == want[5] > 0
    assert o_on["pairs_verified"] + o_on["skipped_floor_mismatch"] == len(kept)
    assert o_off["pairs_verified"] + o_off["skipped_floor_mismatch"] == int(nvalid.sum())
    for key in ("matches", "retrieval_floor_rejected"):
        assert o_on[key] == o_off[key]
    for o in (o_on, o_off):
        assert o["pairs_verified"] == o["verified_valid"] + o["verifier_invalid"]
        assert o["accepted"] == o["verified_valid"] - o["gate_rejected_cross_floor"]
    # every surviving ordered pair: the off run's row for that pair, field by field
    rows_off, rows_on = _pair_rows(g_off), _pair_rows(g_on)
    assert set(rows_on) <= set(kept) and len(rows_on) == o_on["pairs_verified"] > 0
    assert list(zip(g_on.last_pair_results["a"].tolist(), g_on.last_pair_results["b"].tolist())) == \
        [p for p in kept if p in rows_on]  # row-major by query, re-ranked order within a row
    for p, row in rows_on.items():
        assert rows_off[p] == row, p
    assert o_on["accepted"] <= o_off["accepted"]


def test_device_gate_top_k_at_least_k_changes_no_count(gates):
    _, o_off = gates["off"]
    g_all, o_all = gates["all"]
    assert o_all["reranked_out"] == 0
    assert {k: v for k, v in o_all.items() if k not in ("reranked_out", "rerank_candidates")} == o_off
    assert _pair_rows(g_all) == _pair_rows(gates["off"][0])


def test_device_gate_constructor_refusals(dev, gates):
    from mlgate.pipeline import DeviceGate, FullSemanticGate
    frames, seq, labels, kw = gates["frames"], gates["seq"], gates["labels"], gates["kw"]
    for bad in (dict(rerank_top_k=2, local_features=False), dict(rerank_top_k=0), dict(rerank_top_k=2, k=65)):
        with pytest.raises(ValueError):
            DeviceGate(frames, seq.t, labels, **dict(kw, **bad))
    for bad in (dict(rerank_top_k=2, vpr_method="mixvpr"), dict(rerank_top_k=0), dict(rerank_top_k=2, k=65)):
        with pytest.raises(ValueError):
            FullSemanticGate(device=str(dev), **bad)


def test_full_gate_keeps_the_same_pairs(dev, gates):
    from mlgate.pipeline import FullSemanticGate
    from oracle import geometry as ogeo
    kw = gates["kw"]
    g_on, o_on = gates["on"]
    fg = FullSemanticGate(device=str(dev), k=GATE_K, similarity_threshold=kw["similarity_threshold"],
                          min_time_gap=kw["min_time_gap"], retrieval_floor_gating=False, rerank_top_k=GATE_TOP)
    rep = fg.run(gates["frames"], gates["seq"].t, K=ogeo.ISEC_K, floor_labels=gates["labels"])
    r_idx, r_count = g_on.last_rerank[0], g_on.last_rerank[4]
    kept = [(i, int(j)) for i in range(len(r_count)) for j in r_idx[i, :r_count[i]]]
    assert [(m.query_idx, m.match_idx) for m in rep.verified] == kept
    assert len(rep.reranked_out) == o_on["reranked_out"]
    assert len(rep.verified) + len(rep.reranked_out) == sum(1 for m in rep.matches if m.is_valid)
    assert rep.rejections.total == sum(rep.rejections.as_dict()[k] for k in (
        "retrieval_floor_rejected", "skipped_floor_mismatch", "verifier_invalid", "gate_rejected_cross_floor"))
    assert len(rep.accepted) == o_on["accepted"]
