"""The re-ranking selection rule and the ABI's refusals, without a device.

The numpy restatement (tests/rerank_restatement.py) is what the GPU tests compare
mlg_rerank_gate with; here it is held against the reference's own rule (oracle.xcorr.rerank,
the restatement of CricaVPR.rerank_candidates) given the same cross scores, and against the
reference's recorded output (tests/golden/xcorr.npz: rr, rr_nocache).  mlg_rerank_gate
refuses bad arguments before its first HIP call, so the refusals run through ctypes on a
machine without a GPU."""
import ctypes
import os

import numpy as np
import pytest

from oracle import xcorr as oxc
from rerank_restatement import crafted_lists, rerank_rows, row_candidates

GOLD = os.path.join(os.path.dirname(__file__), "golden")
EINVAL, ENOMEM = -1, -3


def _oracle_rows(feats, idx, sim, mask, count, top_k, q0, cached):
    F = len(feats)
    cache = {f: feats[f] for f in range(F) if cached is None or cached[f]}
    return [oxc.rerank(cache, q0 + i, row_candidates(idx, sim, mask, count, i), top_k) for i in range(len(count))]


def _check_rows(got, want):
    r_idx, r_sim, r_cross, r_score, r_count, dropped = got
    for i, row in enumerate(want):
        assert r_count[i] == len(row)
        assert [int(j) for j in r_idx[i, :len(row)]] == [j for j, _ in row]
        assert [float(s) for s in r_score[i, :len(row)]] == [float(s) for _, s in row]
        assert np.all(r_idx[i, len(row):] == -1)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("top_k", [1, 3, 6])
def test_restatement_equals_oracle(seed, top_k):
    feats, idx, sim, mask, count, q0, cached = crafted_lists(seed)
    cross = lambda a, b: oxc.xcorr_score(feats[a], feats[b])  # noqa: E731
    for m, c in ((mask, cached), (None, cached), (mask, None), (None, None)):
        got = rerank_rows(idx, sim, m, count, cross, top_k, q0=q0, cached=c, F=len(feats))
        _check_rows(got, _oracle_rows(feats, idx, sim, m, count, top_k, q0, c))
        ncand = sum(len(row_candidates(idx, sim, m, count, i)) for i in range(len(count)))
        assert got[5] == ncand - int(got[4].sum())
    # the tie keeps emission order: frame 2 (slot 0) before frame 5 (slot 2)
    r_idx = rerank_rows(idx, sim, mask, count, cross, 6, q0=q0, cached=cached, F=len(feats))[0]
    row = [int(j) for j in r_idx[0]]
    assert row.index(2) + 1 == row.index(5)


def test_restatement_out_of_range_index_is_not_cached():
    feats, idx, sim, mask, count, q0, cached = crafted_lists(3)
    idx[4, 1], idx[4, 2] = 9, -3

    def cross(a, b):
        assert 0 <= b < len(feats)
        return oxc.xcorr_score(feats[a], feats[b])
    r_idx, _, r_cross, r_score, r_count, _ = rerank_rows(idx, sim, None, count, cross, 6, q0=q0, cached=None,
                                                         F=len(feats))
    for bad, s in ((9, 1), (-3, 2)):
        pos = [int(j) for j in r_idx[4]].index(bad)
        assert np.isnan(r_cross[4, pos]) and r_score[4, pos] == np.float64(sim[4, s])


def test_restatement_reproduces_the_reference_output():
    """rr / rr_nocache of tests/golden/xcorr.npz are CricaVPR.rerank_candidates' own output."""
    g = dict(np.load(os.path.join(GOLD, "xcorr.npz")))
    feats = g["feats"].astype(np.float32)[:, 0]
    cands = g["cands"]
    k = len(cands)
    idx = np.tile(cands[:, 0].astype(np.int32), (6, 1))
    sim = np.tile(cands[:, 1].astype(np.float32), (6, 1))
    count = np.full(6, k, np.int32)
    cached = np.array([1, 1, 1, 1, 1, 0], np.uint8)
    cross = lambda a, b: oxc.xcorr_score(feats[a], feats[b])  # noqa: E731
    rr = g["rr"]
    gaps = -np.diff(rr[:, 1])
    # the golden's order does not hang on the last bits: its smallest gap (0.0299, between
    # the third and fourth kept entries) is 3000 times the 1e-5 its scores are compared at
    assert gaps.min() >= 0.029
    r_idx, _, _, r_score, r_count, _ = rerank_rows(idx, sim, None, count, cross, 4, cached=cached, F=6)
    assert np.array_equal(r_idx[0], rr[:, 0].astype(np.int32)) and r_count[0] == 4
    # the golden's global similarities are Python floats; the lists carry them as float32:
    # half of a float32 rounding of a value below 1
    assert np.max(np.abs(r_score[0] - rr[:, 1])) < 2.0 ** -25
    r_idx, _, r_cross, r_score, r_count, _ = rerank_rows(idx, sim, None, count, cross, 3, cached=cached, F=6)
    nc = g["rr_nocache"]
    assert np.array_equal(r_idx[5], nc[:, 0].astype(np.int32)) and r_count[5] == 3
    assert np.max(np.abs(r_score[5] - nc[:, 1])) < 2.0 ** -24 and np.all(np.isnan(r_cross[5]))


# ------------------------------------------------------------------ the ABI
@pytest.fixture(scope="module")
def lib():
    from mlgate import _native
    return _native.lib()


def _call(lib, d, **over):
    """mlg_rerank_gate with dummy non-null pointers (never dereferenced: every refusal
    comes before the first HIP call) and a good shape, except what `over` replaces."""
    a = dict(feats=d, F=9, L=35, D=64, q0=2, Q=4, k=8, idx=d, sim=d, mask=d, count=d, cached=d, top_k=3, ws=d,
             ws_bytes=None, r_idx=d, r_sim=d, r_cross=d, r_score=d, r_count=d, dropped=d, stream=None)
    a.update(over)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = max(lib.mlg_rerank_workspace_bytes(a["F"], a["L"], a["D"], a["Q"], a["k"]), 1)
    return lib.mlg_rerank_gate(*(a[n] for n in ("feats", "F", "L", "D", "q0", "Q", "k", "idx", "sim", "mask", "count",
                                              "cached", "top_k", "ws", "ws_bytes", "r_idx", "r_sim", "r_cross",
                                              "r_score", "r_count", "dropped", "stream")))


@pytest.fixture(scope="module")
def d():
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)
    p._keep = buf
    return p


@pytest.mark.parametrize("name", ["feats", "idx", "sim", "count", "ws", "r_idx", "r_sim", "r_cross", "r_score",
                                  "r_count"])
def test_null_required_pointer_is_refused(lib, d, name):
    assert _call(lib, d, **{name: None}) == EINVAL


@pytest.mark.parametrize("over", [dict(top_k=0), dict(top_k=9), dict(k=0, top_k=1), dict(k=65), dict(D=66),
                                  dict(q0=6), dict(q0=-1), dict(F=0), dict(L=0), dict(D=0), dict(Q=0), dict(F=-3),
                                  dict(Q=-1), dict(L=-35)],
                         ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_bad_sizes_are_refused(lib, d, over):
    assert _call(lib, d, **over) == EINVAL


def test_short_workspace_is_refused(lib, d):
    need = lib.mlg_rerank_workspace_bytes(9, 35, 64, 4, 8)
    assert need >= 4 * (9 * 35 * 64 + 4 * 8)
    assert _call(lib, d, ws_bytes=need - 1) == ENOMEM
    assert _call(lib, d, ws_bytes=0) == ENOMEM


@pytest.mark.parametrize("shape", [(0, 35, 64, 4, 8), (9, 0, 64, 4, 8), (9, 35, 0, 4, 8), (9, 35, 64, 0, 8),
                                   (9, 35, 64, 4, 0), (9, 35, 64, 4, 65), (9, 35, 66, 4, 8), (-1, 35, 64, 4, 8)])
def test_workspace_query_is_zero_on_a_bad_shape(lib, shape):
    assert lib.mlg_rerank_workspace_bytes(*shape) == 0


def _a256(x):
    return (x + 255) & ~255


# the workload's shape, small ones, the largest k, odd sizes whose buffers need the rounding
@pytest.mark.parametrize("shape", [(1, 1, 4, 1, 1), (40, 528, 768, 40, 5), (1000, 528, 768, 500, 20),
                                   (5000, 528, 768, 5000, 20), (9, 35, 64, 4, 64), (9, 143, 384, 9, 9),
                                   (3, 7, 12, 5, 3), (6, 4096, 64, 6, 5)])
def test_workspace_size_is_the_documented_layout(lib, shape):
    """include/mlgate.h's layout of the workspace, restated: the normalised bank f32 [F, L, D]
    and the cross score per slot f32 [Q, k], each rounded up to 256 bytes."""
    F, L, D, Q, k = shape
    assert lib.mlg_rerank_workspace_bytes(*shape) == _a256(4 * F * L * D) + _a256(4 * Q * k)


def test_workspace_query_refuses_rows_past_the_lds_maxima(lib):
    assert lib.mlg_rerank_workspace_bytes(6, 4097, 64, 6, 5) == 0
