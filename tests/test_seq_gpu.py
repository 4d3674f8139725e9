"""mlg_seq_gate on the GPU: against the rule restated in numpy float64 (tests/seq_restatement.py)
over mlg_similarity's own matrix, bit for bit; against the float64 restatement from the
descriptors alone; with a poisoned workspace; and the stage inside both composed gates."""
import functools

import numpy as np
import pytest
import torch

import seq_restatement as sr
from mlgate import _native, gate_plan, retrieval

pytestmark = pytest.mark.gpu
N_WALK = len(sr.ORDER)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _walk(D):
    return sr.walk(D)


@functools.lru_cache(maxsize=None)
def _device_S(D):
    """mlg_similarity's matrix of the walk's normalised rows: existing code, the checker."""
    ops = _native.ops()
    xn = ops.row_normalize(torch.from_numpy(_walk(D)[0]).to("cuda:0"))
    S = ops.similarity(xn, xn).cpu().numpy()
    S.setflags(write=False)
    return S


def _floors(n):
    """Labels that change at frames 20 and 70, two unlabelled frames (as vpr.floor_codes
    makes them: a code per distinct label, has = 0 for None)."""
    code = np.where(np.arange(n) < 20, 0, np.where(np.arange(n) < 70, 1, 2)).astype(np.int64)
    has = np.ones(n, np.uint8)
    has[[33, 71]] = 0
    return code, has


def _lists(dev, X, t, code, has, gap, thr, k, q0, Q):
    out = retrieval.knn_gate(_t(X, dev), _t(t, dev), _t(code, dev), _t(has, dev), gap, thr, k, False, q0=q0, Q=Q)
    return [x.cpu().numpy() for x in out]


def _run(dev, X, t, code, has, idx, sim, mask, count, w, thr, gap, min_terms, q0):
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    out = retrieval.sequence_gate(_t(X, dev), _t(t, dev), _t(code, dev), _t(has, dev), _t(idx, dev), _t(sim, dev),
                                  _t(mask, dev), _t(count, dev), w, thr, gap, min_terms, q0=q0, totals=tot)
    return tuple(x.cpu().numpy() for x in out) + (int(tot.item()),)


def _same(got, want):
    for name, g, x in zip(("s_score", "s_dir", "s_terms", "keep"), got, want):
        assert g.dtype == x.dtype and g.shape == x.shape, name
        if name == "s_score":
            bad = np.argwhere(_bits(g) != _bits(x))
            assert len(bad) == 0, (name, bad[:5].tolist(), g[tuple(bad[0])], x[tuple(bad[0])])
        else:
            assert np.array_equal(g, x), (name, np.argwhere(g != x)[:5].tolist())
    assert got[4] == want[4], "rejected total"


# ------------------------------------------------------------------ the exact check
@pytest.mark.parametrize("k", [5, 64])
@pytest.mark.parametrize("w", [1, 3, 7])
@pytest.mark.parametrize("D", [768, 100, 384])  # 100: a ragged last k slab
def test_equals_the_rule_over_mlg_similarity_bit_for_bit(dev, D, w, k):
    """Two calls per shape.  (a) All 96 rows (rows 0 and N - 1 clip their windows), floor
    labels that change at 20 and 70 with two unlabelled frames, a row with count 0, a mask
    with holes, an idx slot set to -1 and one to N.  (b) A rank's slice q0 = 37, Q = 41
    whose windows reach outside it, min_terms = 6 so that some entries pass unjudged."""
    X, t, _ = _walk(D)
    S = _device_S(D)
    code, has = _floors(N_WALK)
    thr = sr.RETRIEVAL_THR if k == 5 else -1.0  # k = 64: full lists, four passes of 16 slots
    # (a)
    idx, sim, _, count = _lists(dev, X, t, code, has, sr.MIN_GAP, thr, k, 0, N_WALK)
    assert count.max() == 64 if k == 64 else 1 < count.max() <= 5
    rng = np.random.default_rng(k + w)
    mask = (rng.random(idx.shape) > 0.2).astype(np.uint8)
    count[50] = 0
    r1, r2 = (int(r) for r in np.flatnonzero(count > 0)[[3, -3]])
    idx[r1, 0], idx[r2, count[r2] - 1] = -1, N_WALK
    mask[r1, 0] = mask[r2, count[r2] - 1] = 1
    want = sr.seq_rows(S, t, code, has, idx, sim, mask, count, w, sr.MIN_GAP, 2, sr.SEQ_THR)
    got = _run(dev, X, t, code, has, idx, sim, mask, count, w, sr.SEQ_THR, sr.MIN_GAP, 2, 0)
    _same(got, want)
    live = (np.arange(k)[None, :] < count[:, None]) & (mask != 0)
    assert got[3][r1, 0] == 0 and got[3][r2, count[r2] - 1] == 0 and not got[3][~live].any()
    assert want[4] < live.sum() and set(np.unique(want[1])) == {-1, 0, 1}
    assert want[4] > 0 or w == 1  # w = 1: a mean of three terms, one of them the alias's ~0.9
    # (b)
    q0, Q = 37, 41
    idx, sim, _, count = _lists(dev, X, t, code, has, sr.MIN_GAP, thr, k, q0, Q)
    none = np.zeros(N_WALK, np.int64), np.zeros(N_WALK, np.uint8)
    for fl, mt in ((none, 2), ((code, has), 6)):
        want = sr.seq_rows(S, t, *fl, idx, sim, None, count, w, sr.MIN_GAP, mt, sr.SEQ_THR, q0=q0)
        _same(_run(dev, X, t, *fl, idx, sim, None, count, w, sr.SEQ_THR, sr.MIN_GAP, mt, q0), want)
        live = np.arange(k)[None, :] < count[:, None]
        if mt == 6:  # w = 1 has 2 terms at most: every candidate passes unjudged; w = 3 needs all 6
            unjudged = live & (want[1] == 0)
            assert np.all(want[3][unjudged] == 1) and (w > 3 or unjudged.any())
            assert w > 1 or unjudged.sum() == live.sum()
            assert np.array_equal(_bits(want[0][unjudged]), _bits(sim[unjudged].astype(np.float64)))


def test_a_map_smaller_than_the_window(dev):
    """N = 3 at w = 3 and w = 7: every window is clipped on both sides."""
    X = np.random.default_rng(3).standard_normal((3, 100)).astype(np.float32)
    t = np.arange(3, dtype=np.float64)
    code, has = np.zeros(3, np.int64), np.zeros(3, np.uint8)
    ops = _native.ops()
    xn = ops.row_normalize(_t(X, dev))
    S = ops.similarity(xn, xn).cpu().numpy()
    idx, sim, _, count = _lists(dev, X, t, code, has, 0.5, -1.0, 3, 0, 3)
    assert count.tolist() == [2, 2, 2]
    for w in (3, 7):
        for mt in (1, 2):
            want = sr.seq_rows(S, t, code, has, idx, sim, None, count, w, 0.5, mt, 0.0)
            _same(_run(dev, X, t, code, has, idx, sim, None, count, w, 0.0, 0.5, mt, 0), want)
    assert want[2].max() <= 2


def test_more_workgroups_than_compute_units(dev):
    """N = 600, k = 8: 600 workgroups on 256 CUs; a repeated call is bit-identical."""
    rng = np.random.default_rng(5)
    N, D, k = 600, 100, 8
    place = np.concatenate([np.arange(200), np.arange(200), np.arange(199, -1, -1)])
    X = (rng.standard_normal((200, D))[place] + 0.35 * rng.standard_normal((N, D))).astype(np.float32)
    t = np.arange(N, dtype=np.float64)
    code, has = (np.arange(N) // 150).astype(np.int64), (rng.random(N) > 0.05).astype(np.uint8)
    ops = _native.ops()
    xn = ops.row_normalize(_t(X, dev))
    S = ops.similarity(xn, xn).cpu().numpy()
    idx, sim, _, count = _lists(dev, X, t, code, has, 5.0, 0.2, k, 0, N)
    mask = (rng.random(idx.shape) > 0.1).astype(np.uint8)
    want = sr.seq_rows(S, t, code, has, idx, sim, mask, count, 3, 5.0, 2, 0.3)
    got = _run(dev, X, t, code, has, idx, sim, mask, count, 3, 0.3, 5.0, 2, 0)
    _same(got, want)
    again = _run(dev, X, t, code, has, idx, sim, mask, count, 3, 0.3, 5.0, 2, 0)
    for a, b in zip(got[:4], again[:4]):
        assert a.tobytes() == b.tobytes()
    assert got[4] == again[4] > 0 and want[3].sum() > 0


# ------------------------------------------------------------ the independent check
@pytest.mark.parametrize("D", [768, 384, 100])
def test_against_float64_from_the_descriptors_alone(dev, D):
    """The restatement over a float64 similarity matrix made from the descriptors with numpy
    (centre term included), the retrieval's lists giving only which entries exist.  Bar:
    |s_score - ref| <= 4e-6, the project's bar for a float32 similarity against the oracle; a
    mean of such terms stays within it.  The decision is compared at the midpoint of the
    largest gap of the restated scores (asserted > 1e-4), on every entry.
    Measured on an MI355X: max |s_score - ref| 2.8e-7 / 2.0e-7 / 1.0e-7 and a largest gap of
    0.190 / 0.196 / 0.223 at D = 768 / 384 / 100."""
    X, t, _ = _walk(D)
    S64 = sr.similarity64(X)
    none = np.zeros(N_WALK, np.int64), np.zeros(N_WALK, np.uint8)
    idx, sim, _, count = _lists(dev, X, t, *none, sr.MIN_GAP, sr.RETRIEVAL_THR, sr.K, 0, N_WALK)
    live = np.arange(sr.K)[None, :] < count[:, None]
    assert live.sum() == 158
    sim64 = np.where(live, S64[np.arange(N_WALK)[:, None], np.clip(idx, 0, N_WALK - 1)], 0.0)
    ref = sr.seq_rows(S64, t, *none, idx, sim64, None, count, sr.W, sr.MIN_GAP, 2, sr.SEQ_THR)
    scores = np.sort(ref[0][live])
    gaps = np.diff(scores)
    g = int(np.argmax(gaps))
    thr = 0.5 * (scores[g] + scores[g + 1])
    print(f"D = {D}: largest gap {gaps[g]:.4f} at {thr:.4f}")
    assert gaps[g] > 1e-4
    ref = sr.seq_rows(S64, t, *none, idx, sim64, None, count, sr.W, sr.MIN_GAP, 2, thr)
    got = _run(dev, X, t, *none, idx, sim, None, count, sr.W, thr, sr.MIN_GAP, 2, 0)
    err = np.abs(got[0] - ref[0]).max()
    print(f"D = {D}: max |s_score - ref| = {err:.3e}")
    assert err <= 4e-6
    assert np.array_equal(got[3], ref[3]) and got[4] == ref[4] == 12
    assert np.array_equal(got[2], ref[2])
    alias = np.array([f for f, _ in sr.ALIASES])
    touch = live & (np.isin(np.arange(N_WALK), alias)[:, None] | np.isin(idx, alias))
    assert np.array_equal(got[3] != 0, live & ~touch)  # every true revisit kept, every alias entry rejected


# ------------------------------------------------------------ the poisoned workspace
def test_poisoned_workspace_changes_nothing(dev):
    """mlg_seq_gate through the C ABI on a workspace of 0xFF bytes (NaN as f32), of zeros, and
    the operator's own: the same bits every time."""
    X, t, _ = _walk(100)
    code, has = _floors(N_WALK)
    q0, Q, k = 37, 41, 5
    idx, sim, valid, count = _lists(dev, X, t, code, has, sr.MIN_GAP, sr.RETRIEVAL_THR, k, q0, Q)
    want = _run(dev, X, t, code, has, idx, sim, valid, count, sr.W, sr.SEQ_THR, sr.MIN_GAP, 2, q0)
    L = _native.lib()
    ins = [_t(a, dev) for a in (X, t, code, has, idx, sim, valid, count)]
    need = L.mlg_seq_workspace_bytes(N_WALK, 100, Q, k)
    p = _native.ptr
    runs = []
    for fill in (255, 255, 0):
        ws = torch.full((need,), fill, dtype=torch.uint8, device=dev)
        outs = [torch.empty(Q, k, dtype=d, device=dev) for d in (torch.float64, torch.int8, torch.int32, torch.uint8)]
        tot = torch.zeros(1, dtype=torch.int64, device=dev)
        rc = L.mlg_seq_gate(p(ins[0]), N_WALK, 100, p(ins[1]), p(ins[2]), p(ins[3]), q0, Q, k, p(ins[4]), p(ins[5]),
                            p(ins[6]), p(ins[7]), sr.W, sr.MIN_GAP, 2, sr.SEQ_THR, p(ws), need, p(outs[0]), p(outs[1]),
                            p(outs[2]), p(outs[3]), p(tot), _native.stream_of(dev))
        assert rc == 0
        torch.cuda.synchronize(dev)
        runs.append([o.cpu().numpy().tobytes() for o in outs] + [int(tot.item())])
    assert runs[0] == runs[1] == runs[2]
    assert runs[0] == [a.tobytes() for a in want[:4]] + [want[4]]


def test_python_refusals(dev):
    z = torch.zeros
    desc, t = z(4, 8, device=dev), z(4, dtype=torch.float64, device=dev)
    fl, hf = z(4, dtype=torch.int64, device=dev), z(4, dtype=torch.uint8, device=dev)
    idx, sim, count = z(2, 3, dtype=torch.int32, device=dev), z(2, 3, device=dev), z(2, dtype=torch.int32, device=dev)
    for bad in (dict(radius=0), dict(radius=8), dict(min_terms=0)):
        kw = dict(dict(radius=3, threshold=0.3, min_gap=1.0), **bad)
        with pytest.raises(ValueError):
            retrieval.sequence_gate(desc, t, fl, hf, idx, sim, None, count, **kw)
    with pytest.raises(ValueError):
        retrieval.sequence_gate(desc, t, fl, hf, z(2, 65, dtype=torch.int32, device=dev), z(2, 65, device=dev), None,
                                count, 3, 0.3, 1.0)
    with pytest.raises(RuntimeError):
        retrieval.sequence_gate(desc, t, fl, hf, idx, sim, None, count, 3, 0.3, 1.0, q0=3)  # q0 + Q > N


# ------------------------------------------------------------- inside the gates
class WalkEngine:
    """Stands in for the gate's ViT engine: writes rows [lo, hi) of the walk's descriptors
    (and seeded local features) where the forward would write its own, so that DeviceGate's
    retrieval sees the 96 frames of the walk.  Everything after the descriptors is the gate's
    own code."""

    def __init__(self, eng, lo, hi):
        self.n_local = eng.n_local
        self.rows = torch.from_numpy(_walk(768)[0][lo:hi])

    def forward_into(self, frames, desc_out, local_out=None):
        desc_out.copy_(self.rows.to(desc_out.device))
        if local_out is not None:
            g = torch.Generator(device=local_out.device).manual_seed(7)
            local_out.copy_(torch.randn(local_out.shape, generator=g, device=local_out.device))


def walk_gate(dev, world=1, rank=0, **kw):
    from mlgate import distributed as mdist
    from mlgate.pipeline import DeviceGate
    lo, hi = mdist.shard(N_WALK, world, rank)
    frames = torch.zeros(hi - lo, 8, 8, 3, dtype=torch.uint8, device=dev)
    kw = dict(dict(k=sr.K, similarity_threshold=sr.RETRIEVAL_THR, min_time_gap=sr.MIN_GAP, verify=False, record=True,
                   local_features=False, vit_batch=8), **kw)
    g = DeviceGate(frames, _walk(768)[1], np.zeros(N_WALK, np.int64), world, rank, dev, **kw)
    g.eng = WalkEngine(g.eng, lo, hi)
    return g


PARENT_KEYS = ("matches", "retrieval_floor_rejected", "skipped_floor_mismatch", "verifier_invalid",
               "gate_rejected_cross_floor", "pairs_verified", "verified_valid", "accepted")


@pytest.fixture(scope="module")
def gates(dev):
    out = {}
    for name, kw in (("off", {}), ("on", dict(seq_radius=sr.W, seq_threshold=sr.SEQ_THR))):
        g = walk_gate(dev, **kw)
        out[name] = (g, g.step())
    return out


def test_device_gate_runs_the_stage_after_retrieval(dev, gates):
    g, o = gates["on"]
    h_idx, h_sim, h_valid, h_count = g.last_retrieval
    X, t, _ = _walk(768)
    none = np.zeros(N_WALK, np.int64), np.ones(N_WALK, np.uint8)  # every frame labelled floor 0
    by_hand = _run(dev, X, t, *none, h_idx, h_sim, h_valid, h_count, sr.W, sr.SEQ_THR, sr.MIN_GAP, 2, 0)
    assert len(g.last_sequence) == 4
    for a, b in zip(g.last_sequence, by_hand[:4]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    want = sr.seq_rows(_device_S(768), t, *none, h_idx, h_sim, h_valid, h_count, sr.W, sr.MIN_GAP, 2, sr.SEQ_THR)
    assert o["sequence_rejected"] == want[4] == by_hand[4] == 12
    assert o["sequence_candidates"] == 158 == o["matches"] - o["retrieval_floor_rejected"]
    pa, pb = gate_plan.pairs_from_sequence(h_idx, g.last_sequence[3], 0)
    assert len(pa) == 146 and np.array_equal(g.last_pairs[0], pa) and np.array_equal(g.last_pairs[1], pb)
    assert set(o) == set(PARENT_KEYS) | {"sequence_candidates", "sequence_rejected"}


def test_device_gate_without_the_stage_is_the_parent(gates):
    g, o = gates["off"]
    h_idx, _, h_valid, h_count = g.last_retrieval
    matches, floor_rej, pa, pb = gate_plan.pairs_from_retrieval(h_idx, h_valid, h_count, 0)
    assert tuple(o) == PARENT_KEYS  # key for key, in the parent's order
    assert o == dict.fromkeys(PARENT_KEYS, 0) | {"matches": matches, "retrieval_floor_rejected": floor_rej}
    assert g.last_sequence is None and len(pa) == 158
    assert np.array_equal(g.last_pairs[0], pa) and np.array_equal(g.last_pairs[1], pb)
    on = gates["on"][0]
    for a, b in zip(g.last_retrieval, on.last_retrieval):  # the retrieval lists are unchanged
        assert a.tobytes() == b.tobytes()


def test_rerank_gets_the_kept_entries_as_its_mask(dev, gates, monkeypatch):
    seen = {}
    real = retrieval.rerank_gate

    def spy(feats, idx, sim, mask, count, top_k, **kw):
        seen["mask"] = mask.cpu().numpy().copy()
        return real(feats, idx, sim, mask, count, top_k, **kw)

    monkeypatch.setattr(retrieval, "rerank_gate", spy)
    g = walk_gate(dev, seq_radius=sr.W, seq_threshold=sr.SEQ_THR, rerank_top_k=1, local_features=True)
    o = g.step()
    h_idx, _, h_valid, h_count = g.last_retrieval
    keep = g.last_sequence[3]
    live = np.arange(sr.K)[None, :] < h_count[:, None]
    assert seen["mask"].dtype == np.uint8
    assert np.array_equal(seen["mask"] != 0, live & (h_valid != 0) & (keep != 0))
    assert g.last_sequence[3].tobytes() == gates["on"][0].last_sequence[3].tobytes()
    assert o["sequence_candidates"] == 158 and o["sequence_rejected"] == 12 and o["rerank_candidates"] == 146
    rows = int((keep != 0).any(1).sum())  # top_k = 1: one pair per row that kept any
    assert len(g.last_pairs[0]) == rows == o["rerank_candidates"] - o["reranked_out"]
    kept = set(zip(*(a.tolist() for a in gate_plan.pairs_from_sequence(h_idx, keep, 0))))
    assert set(zip(g.last_pairs[0].tolist(), g.last_pairs[1].tolist())) <= kept


def test_full_gate_reports_the_rejected_matches(dev):
    """FullSemanticGate(seq_radius=3) on 12 small frames: the threshold is the median of the
    scores the op gives by hand on the gate's own descriptors, so both lists are non-empty."""
    from mlgate import synthetic
    from mlgate.pipeline import FullSemanticGate
    from mlgate.vpr import SemanticPlaceRecognition, floor_codes
    from oracle import geometry as ogeo
    seq = synthetic.make_sequence(12, 4, 3, ((5, 1.0),))
    frames = torch.from_numpy(synthetic.frames_host(seq, h=240, w=320)).to(dev)
    labels = [5] * 12
    kw = dict(device=str(dev), k=4, similarity_threshold=-1.0, min_time_gap=1.0)
    spr = SemanticPlaceRecognition("cricavpr", str(dev), -1.0, 1.0)
    spr.add_images(frames, seq.t.tolist(), labels)
    ms = [m for m in spr.find_loop_closures(k=4) if m.is_valid]
    X, d = spr.vpr._device_matrix()
    codes, has = floor_codes(labels)
    idx = np.array([m.match_idx for m in ms], np.int32).reshape(12, 4)
    sim = np.array([m.similarity for m in ms], np.float32).reshape(12, 4)
    s_score, _, s_terms, _ = retrieval.sequence_gate(
        X, _t(seq.t, d), _t(codes, d), _t(has, d), _t(idx, d), _t(sim, d), None,
        _t(np.full(12, 4, np.int32), d), 3, 0.0, 1.0)
    s_score, s_terms = s_score.cpu().numpy(), s_terms.cpu().numpy()
    thr = float(np.median(s_score[s_terms > 0]))
    fg = FullSemanticGate(seq_radius=3, seq_threshold=thr, **kw)
    rep = fg.run(frames, seq.t, K=ogeo.ISEC_K, floor_labels=labels)
    valid = [(m.query_idx, m.match_idx) for m in rep.matches if m.is_valid]
    assert len(valid) == 48
    rej = [(m.query_idx, m.match_idx) for m in rep.sequence_rejected]
    ver = [(m.query_idx, m.match_idx) for m in rep.verified]
    assert len(rej) > 0 and len(ver) > 0 and not set(rej) & set(ver)
    assert sorted(rej + ver) == sorted(valid) and [p for p in valid if p in set(ver)] == ver
    want_rej = [(i, int(idx[i, s])) for i in range(12) for s in range(4) if s_terms[i, s] > 0 and s_score[i, s] < thr]
    assert rej == want_rej
    assert rep.rejections.total == sum(rep.rejections.as_dict()[k_] for k_ in (
        "retrieval_floor_rejected", "skipped_floor_mismatch", "verifier_invalid", "gate_rejected_cross_floor"))
    assert rep.reranked_out == []
