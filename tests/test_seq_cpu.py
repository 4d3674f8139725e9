"""The sequence-consistency rule, DeviceGate's host plan for it and the ABI's refusals,
without a device.

The numpy restatement (tests/seq_restatement.py) is what the GPU tests compare mlg_seq_gate
with; here it runs on the synthetic walk (an outward leg, a forward revisit, a reverse
revisit, four planted one-frame aliases) and must separate the true revisits from the
aliases.  mlg_seq_gate refuses bad arguments before its first HIP call, so the refusals run
through ctypes on a machine without a GPU, with pointers that would fault if read."""
import ctypes

import numpy as np
import pytest

import seq_restatement as sr

EINVAL, ENOMEM = -1, -3


# ------------------------------------------------------------------ the rule
@pytest.fixture(scope="module", params=[768, 384, 100])
def judged(request):
    X, t, _ = sr.walk(request.param)
    S = sr.similarity64(X)
    idx, sim, count = sr.knn_lists(S, t, sr.MIN_GAP, sr.RETRIEVAL_THR, sr.K)
    none = np.zeros(len(t), np.int64), np.zeros(len(t), np.uint8)
    out = sr.seq_rows(S, t, *none, idx, sim, None, count, sr.W, sr.MIN_GAP, 2, sr.SEQ_THR)
    live = np.arange(sr.K)[None, :] < count[:, None]
    alias = np.array([f for f, _ in sr.ALIASES])
    touch = live & (np.isin(np.arange(len(t)), alias)[:, None] | np.isin(idx, alias))
    return dict(idx=idx, sim=sim, count=count, live=live, touch=touch, out=out)


def test_true_revisits_are_kept_and_aliases_rejected(judged):
    s_score, s_dir, s_terms, keep, rejected = judged["out"]
    live, touch = judged["live"], judged["touch"]
    true = live & ~touch
    print(f"emitted {live.sum()}, true {true.sum()} (min score {s_score[true].min():.4f}), alias entries "
          f"{touch.sum()} (max score {s_score[touch].max():.4f}, single-frame sim {judged['sim'][touch].min():.3f}"
          f" .. {judged['sim'][touch].max():.3f})")
    assert live.sum() == 158 and true.sum() == 146 and touch.sum() == 12
    assert np.all(judged["sim"][touch] >= sr.RETRIEVAL_THR)  # the aliases pass the retrieval
    assert np.all(keep[true] == 1) and np.all(keep[touch] == 0) and rejected == 12
    assert np.all(keep[~live] == 0) and np.all(s_score[~live] == 0) and np.all(s_dir[~live] == 0)
    assert s_score[true].min() - s_score[touch].max() > 0.15  # one threshold separates the groups
    assert np.all(s_terms[live] >= 2)


def test_direction_follows_the_leg(judged):
    """+1 on the forward revisit, -1 on the reverse one; the outward leg's frames are found by
    both legs, so their entries carry both directions."""
    _, s_dir, _, keep, _ = judged["out"]
    true = judged["live"] & ~judged["touch"]
    idx = judged["idx"]
    outward = idx < 40  # the match is a frame of the outward leg
    fwd = true[list(sr.FORWARD)] & outward[list(sr.FORWARD)]
    rev = true[list(sr.REVERSE)] & outward[list(sr.REVERSE)]
    assert fwd.sum() > 20 and rev.sum() > 20
    assert np.all(s_dir[list(sr.FORWARD)][fwd] == 1)
    assert np.all(s_dir[list(sr.REVERSE)][rev] == -1)
    assert {-1, 1} <= set(s_dir[true].tolist())


def test_rule_edges_by_hand():
    """A 7-frame map with a hand-made similarity table: clipping at the ends, the time mask,
    the floor rule, min_terms, the tie, non-candidates."""
    N = 7
    S = np.full((N, N), 0.25)
    t = np.arange(N, dtype=np.float64) * 10
    code, has = np.zeros(N, np.int64), np.zeros(N, np.uint8)
    idx = np.array([[6, 5, -1, 7]], np.int32)
    sim = np.array([[0.75, 0.5, 0.9, 0.9]], np.float32)
    count = np.array([4], np.int32)
    # query frame 0, w = 2: d = -1, -2 fall off the map; dir +1 reaches j + d = 7, 8: no term
    # for j = 6; dir -1 has (1, 5), (2, 4): two terms of 0.25
    sc, dr, tm, kp, rej = sr.seq_rows(S, t, code, has, idx, sim, None, count, 2, 5.0, 2, 0.4)
    assert dr[0].tolist() == [-1, -1, 0, 0] and tm[0].tolist() == [2, 2, 0, 0]
    assert sc[0, 0] == (0.75 + 0.5) / 3 and sc[0, 1] == (0.5 + 0.5) / 3
    assert kp[0].tolist() == [1, 0, 0, 0] and rej == 1 and sc[0, 2] == sc[0, 3] == 0
    # j = 5: dir +1 has one term (1, 6), dir -1 two; min_terms = 3 leaves neither eligible
    sc, dr, tm, kp, rej = sr.seq_rows(S, t, code, has, idx, sim, None, count, 2, 5.0, 3, 0.4)
    assert kp[0].tolist() == [1, 1, 0, 0] and dr[0].tolist() == [0] * 4 and rej == 0
    assert sc[0, 0] == np.float64(np.float32(0.75))
    # the mask takes an entry out; a count past k is clamped
    mask = np.array([[0, 1, 1, 1]], np.uint8)
    sc, dr, tm, kp, rej = sr.seq_rows(S, t, code, has, idx, sim, mask, np.array([9], np.int32), 2, 5.0, 2, 0.4)
    assert kp[0].tolist() == [0, 0, 0, 0] and sc[0, 0] == 0 and rej == 1
    # the time mask: with min_gap 45 the pairs (1, 5) and (2, 4) are 40 and 20 apart: no term
    sc, dr, tm, kp, rej = sr.seq_rows(S, t, code, has, idx[:, :1], sim[:, :1], None, count[:1] * 0 + 1, 2, 45.0, 1, 0.4)
    assert dr[0, 0] == 0 and kp[0, 0] == 1
    # the floor rule: frame 1 labelled onto another floor than frame 0 drops the term (1, 5)
    has2, code2 = np.ones(N, np.uint8), np.array([0, 1, 0, 0, 0, 0, 0], np.int64)
    sc, dr, tm, kp, rej = sr.seq_rows(S, t, code2, has2, idx[:, :1], sim[:, :1], None, np.array([1], np.int32), 2,
                                      5.0, 1, 0.4)
    assert tm[0, 0] == 1 and dr[0, 0] == -1
    has2[1] = 0  # unlabelled: no objection
    assert sr.seq_rows(S, t, code2, has2, idx[:, :1], sim[:, :1], None, np.array([1], np.int32), 2, 5.0, 1,
                       0.4)[2][0, 0] == 2
    # a tie between the directions goes to +1 (query 3, match 3 is barred by no rule here)
    mid = sr.seq_rows(S, np.arange(N) * 0.0, code, has, np.array([[3]], np.int32), np.array([[0.5]], np.float32),
                      None, np.array([1], np.int32), 1, -1.0, 2, 0.0, q0=3)
    assert mid[1][0, 0] == 1 and mid[2][0, 0] == 2


# ---------------------------------------------------------------- the host plan
def test_pairs_from_sequence():
    from mlgate import gate_plan
    h_idx = np.array([[7, 3, 9], [1, 0, 0], [4, 4, 2]], np.int32)
    keep = np.array([[1, 0, 1], [0, 0, 0], [0, 1, 1]], np.uint8)
    pa, pb = gate_plan.pairs_from_sequence(h_idx, keep, 10)
    assert pa.dtype == pb.dtype == np.int32
    assert pa.tolist() == [10, 10, 12, 12] and pb.tolist() == [7, 9, 4, 2]
    pa, pb = gate_plan.pairs_from_sequence(h_idx, np.zeros_like(keep), 0)
    assert len(pa) == len(pb) == 0
    # with every candidate kept, the plan is the retrieval's own
    valid = np.array([[1, 1, 0], [1, 0, 0], [1, 1, 1]], np.uint8)
    count = np.array([3, 1, 2], np.int32)
    live = np.arange(3)[None, :] < count[:, None]
    _, _, ra, rb = gate_plan.pairs_from_retrieval(h_idx, valid, count, 5)
    pa, pb = gate_plan.pairs_from_sequence(h_idx, (live & (valid != 0)).astype(np.uint8), 5)
    assert pa.tolist() == ra.tolist() and pb.tolist() == rb.tolist()


def test_gate_arguments_are_refused_before_anything_is_built():
    from mlgate.pipeline import DeviceGate, FullSemanticGate
    for bad in (dict(seq_radius=0), dict(seq_radius=8), dict(seq_radius=3, k=65), dict(seq_radius=3, seq_min_terms=0)):
        with pytest.raises(ValueError):
            FullSemanticGate(**bad)
        with pytest.raises(ValueError):  # no frames, no device: the refusal comes first
            DeviceGate(None, [0.0, 1.0], [0, 0], **bad)
    g = FullSemanticGate(seq_radius=3)
    assert (g.seq_radius, g.seq_threshold, g.seq_min_terms) == (3, 0.3, 2)
    assert FullSemanticGate().seq_radius is None


# ------------------------------------------------------------------ the ABI
@pytest.fixture(scope="module")
def lib():
    from mlgate import _native
    return _native.lib()


POISON = ctypes.c_void_p(0xDEAD0000)  # unmapped: a read or a write through it faults


def _call(lib, **over):
    a = dict(desc=POISON, N=96, D=100, t=POISON, floor=POISON, has=POISON, q0=37, Q=41, k=5, idx=POISON, sim=POISON,
             mask=POISON, count=POISON, radius=3, min_gap=5.0, min_terms=2, threshold=0.3, ws=POISON, ws_bytes=None,
             s_score=POISON, s_dir=POISON, s_terms=POISON, keep=POISON, rejected=POISON, stream=None)
    a.update(over)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = max(lib.mlg_seq_workspace_bytes(a["N"], a["D"], a["Q"], a["k"]), 1)
    return lib.mlg_seq_gate(*(a[n] for n in ("desc", "N", "D", "t", "floor", "has", "q0", "Q", "k", "idx", "sim",
                                             "mask", "count", "radius", "min_gap", "min_terms", "threshold", "ws",
                                             "ws_bytes", "s_score", "s_dir", "s_terms", "keep", "rejected",
                                             "stream")))


@pytest.mark.parametrize("name", ["desc", "t", "floor", "has", "idx", "sim", "count", "ws", "s_score", "s_dir",
                                  "s_terms", "keep"])
def test_null_required_pointer_is_refused(lib, name):
    assert _call(lib, **{name: None}) == EINVAL


@pytest.mark.parametrize("over", [dict(N=0), dict(D=0), dict(Q=0), dict(N=-96), dict(D=-1), dict(Q=-41), dict(k=0),
                                  dict(k=65), dict(k=-1), dict(radius=0), dict(radius=8), dict(radius=-3),
                                  dict(min_terms=0), dict(min_terms=-2), dict(q0=-1), dict(q0=56), dict(q0=96)],
                         ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_bad_sizes_are_refused(lib, over):
    assert _call(lib, **over) == EINVAL


def test_short_workspace_is_refused(lib):
    need = lib.mlg_seq_workspace_bytes(96, 100, 41, 5)
    assert need >= 4 * 96 * 100
    assert _call(lib, ws_bytes=need - 1) == ENOMEM
    assert _call(lib, ws_bytes=0) == ENOMEM


@pytest.mark.parametrize("shape", [(0, 100, 41, 5), (96, 0, 41, 5), (96, 100, 0, 5), (96, 100, 41, 0),
                                   (96, 100, 41, 65), (-1, 100, 41, 5), (96, 100, 2**30, 4)])
def test_workspace_query_is_zero_on_a_bad_shape(lib, shape):
    assert lib.mlg_seq_workspace_bytes(*shape) == 0 == sr.seq_workspace_bytes(*shape)


# the measured shape, the walk's, the largest k, odd sizes whose buffer needs the rounding
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (96, 768, 96, 5), (96, 100, 41, 5), (5000, 768, 5000, 20),
                                   (600, 100, 600, 8), (3, 100, 3, 64), (7, 13, 5, 3), (19163, 768, 2396, 10)])
def test_workspace_size_is_the_documented_layout(lib, shape):
    N, D, Q, k = shape
    assert lib.mlg_seq_workspace_bytes(*shape) == sr.seq_workspace_bytes(*shape) == (4 * N * D + 255) // 256 * 256
