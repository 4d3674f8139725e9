"""mlg_knn_append's refusals through ctypes: every one is decided before any HIP call, so they
run without a GPU (the pointers below are never dereferenced)."""
import ctypes

from mlgate import _native

EINVAL, ENOMEM = -1, -3
P = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(12)]   # aligned, non-null, never read


def call(n_old=8, n_new=12, D=64, k=5, gating=1, ws_bytes=None, null=None, misalign=None):
    L = _native.lib()
    if ws_bytes is None:
        ws_bytes = max(int(L.mlg_knn_append_workspace_bytes(n_old, n_new, D, k)), 1)
    names = ["xn", "t", "floor", "has_floor", "ws", "idx", "sim", "valid", "count", "inserted", "evicted", "n_evicted"]
    p = dict(zip(names, P))
    if null:
        p[null] = ctypes.c_void_p(0)
    if misalign:
        p[misalign] = ctypes.c_void_p(p[misalign].value + 2)
    return L.mlg_knn_append(p["xn"], n_old, n_new, D, p["t"], p["floor"], p["has_floor"], 10.0, 0.1, k, gating,
                            p["ws"], ws_bytes, p["idx"], p["sim"], p["valid"], p["count"], p["inserted"],
                            p["evicted"], p["n_evicted"], None)


def test_export_is_declared():
    assert "mlg_knn_append" in _native.EXPORTS and "mlg_knn_append_workspace_bytes" in _native.EXPORTS
    assert "knn_append" in _native.OPS
    assert _native.lib().mlg_abi_version() == 3


def test_domain_refusals():
    assert call(k=33) == EINVAL
    assert call(k=0) == EINVAL
    assert call(D=6) == EINVAL
    assert call(n_old=12, n_new=12) == EINVAL
    assert call(n_old=13, n_new=12) == EINVAL
    assert call(n_old=-1, n_new=3) == EINVAL


def test_phase_selector_refusals():
    L = _native.lib()
    args = [P[0], 8, 12, 64, P[1], P[2], P[3], 10.0, 0.1, 5, 1, P[4], 1 << 20] + P[5:12]
    for phases in (0, 4, -1):
        assert L.mlg_op_knn_append_phases(*args, phases, None) == EINVAL
    assert L.mlg_op_knn_append_phases(*(args[:9] + [33] + args[10:]), 3, None) == EINVAL


def test_pointer_refusals():
    for name in ("idx", "sim", "valid", "count", "xn", "t", "ws", "inserted", "evicted", "n_evicted"):
        assert call(null=name) == EINVAL, name
    assert call(null="floor", gating=1) == EINVAL
    assert call(null="has_floor", gating=1) == EINVAL
    for name in ("xn", "t", "idx", "sim", "count"):
        assert call(misalign=name) == EINVAL, name


def test_workspace_query_and_short_workspace():
    L = _native.lib()
    need = int(L.mlg_knn_append_workspace_bytes(8, 12, 64, 5))
    assert need > 0
    assert call(ws_bytes=need - 1) == ENOMEM
    # the query refuses what the call refuses
    assert L.mlg_knn_append_workspace_bytes(8, 12, 64, 33) == 0
    assert L.mlg_knn_append_workspace_bytes(8, 12, 6, 5) == 0
    assert L.mlg_knn_append_workspace_bytes(12, 12, 64, 5) == 0
    # the update's partial lists grow with the old rows, the fresh rows' with the new ones
    assert int(L.mlg_knn_append_workspace_bytes(4000, 4008, 64, 5)) > need
    assert int(L.mlg_knn_append_workspace_bytes(0, 12, 64, 5)) > 0
