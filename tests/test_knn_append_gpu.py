"""mlg_knn_append / retrieval.StreamingKnn on the GPU: after any sequence of appends the state
holds bit for bit what retrieval.knn_gate returns on the keyframes appended so far
(include/mlgate.h states the rule).  Every comparison is exact: indices, similarities as int32
bits, floor bits, counts, and the memory the call must not write.

Shapes sit around the kernel's 64-row blocks, 16 rows per wave, 128-column tiles, 512-column
splits of the window and 32 list lanes; D = 64 keeps a case at milliseconds."""
import numpy as np
import pytest
import torch

from mlgate import retrieval

pytestmark = pytest.mark.gpu

MIN_GAP = 10.0           # seconds: at 0.765 s per keyframe a band of +-13 keyframes is masked
SENT_I, SENT_BITS, SENT_U8 = -7, 0x5A5A5A5A, 0xAB


def make_inputs(n, D, seed):
    """Seeded descriptors with every fifth row a copy of an earlier one (exact similarity ties,
    also across any old / new boundary), timestamps 0.765 s apart, labels on three floors with
    a quarter of them missing, and a threshold about 1.6 sigma of a random pair's cosine, which
    drops most columns and leaves short lists at small n."""
    rng = np.random.default_rng(seed)
    desc = rng.standard_normal((n, D)).astype(np.float32)
    for i in range(5, n, 5):
        desc[i] = desc[rng.integers(0, i)]
    t = 1000.0 + 0.765 * np.arange(n)
    floor = rng.integers(0, 3, n).astype(np.int64)
    has = (rng.random(n) > 0.25).astype(np.uint8)
    return desc, t, floor, has, float(np.float32(1.6 / np.sqrt(D)))


def to_dev(dev, *arrays):
    return [torch.from_numpy(a).to(dev) for a in arrays]


def new_state(dev, capacity, D, k, thr, gating):
    st = retrieval.StreamingKnn(capacity, D, k, MIN_GAP, thr, gating, device=dev)
    st.idx.fill_(SENT_I)
    st.sim.view(torch.int32).fill_(SENT_BITS)
    st.valid.fill_(SENT_U8)
    st.count.fill_(SENT_I)
    return st


def assert_state_is_batch(st, dev_in, thr, gating):
    """Rows [0, n) equal knn_gate on the first n keyframes; everything else is the sentinel."""
    n, k = st.n, st.k
    desc, t, floor, has = (x[:n] for x in dev_in)
    ridx, rsim, rvalid, rcount = retrieval.knn_gate(desc, t, floor, has, MIN_GAP, thr, k, gating)
    assert torch.equal(st.count[:n], rcount)
    live = torch.arange(k, device=rcount.device)[None, :] < rcount[:, None]
    assert torch.equal(st.idx[:n][live], ridx[live])
    assert torch.equal(st.sim[:n].view(torch.int32)[live], rsim.view(torch.int32)[live])
    assert torch.equal(st.valid[:n][live], rvalid[live])
    # past each row's count, and past row n: never written
    assert bool((st.idx[:n][~live] == SENT_I).all())
    assert bool((st.sim[:n].view(torch.int32)[~live] == SENT_BITS).all())
    assert bool((st.valid[:n][~live] == SENT_U8).all())
    assert bool((st.idx[n:] == SENT_I).all()) and bool((st.sim[n:].view(torch.int32) == SENT_BITS).all())
    assert bool((st.valid[n:] == SENT_U8).all()) and bool((st.count[n:] == SENT_I).all())


def snapshot(st):
    return [x.clone() for x in (st.idx, st.sim.view(torch.int32), st.valid, st.count)]


def assert_difference(before, st, n_old, out):
    """inserted / evicted_idx / n_evicted are the set difference of each old row's list before
    and after, evictions in their former order; an untouched row is bit for bit the snapshot."""
    inserted, evicted, n_evicted = (x.cpu().numpy() for x in out)
    bidx, bsim, bvalid, bcount = (x.cpu().numpy() for x in before)
    aidx, asim, avalid, acount = (x.cpu().numpy() for x in snapshot(st))
    assert inserted.shape == (n_old,) and n_evicted.shape == (n_old,) and evicted.shape == (n_old, st.k)
    for r in range(n_old):
        was, now = list(bidx[r, :bcount[r]]), list(aidx[r, :acount[r]])
        assert inserted[r] == len([j for j in now if j not in was]), r
        gone = [j for j in was if j not in now]
        assert n_evicted[r] == len(gone) and list(evicted[r, :len(gone)]) == gone, r
        assert all(j >= n_old for j in now if j not in was), r
        if inserted[r] == 0:
            assert n_evicted[r] == 0
            for b, a in ((bidx, aidx), (bsim, asim), (bvalid, avalid)):
                assert np.array_equal(b[r], a[r]), r
            assert bcount[r] == acount[r]
    return inserted, bcount, acount


def run_case(dev, n_old, B, k, gating, D=64, seed=0):
    n = n_old + B
    desc, t, floor, has, thr = make_inputs(n, D, seed)
    dev_in = to_dev(dev, desc, t, floor, has)
    st = new_state(dev, n + 3, D, k, thr, gating)
    if n_old:
        out0 = st.append(*(x[:n_old] for x in dev_in))
        assert out0[0].numel() == 0
        assert_state_is_batch(st, dev_in, thr, gating)
    before = snapshot(st)
    out = st.append(*(x[n_old:n] for x in dev_in))
    assert_state_is_batch(st, dev_in, thr, gating)
    return assert_difference(before, st, n_old, out)


@pytest.mark.parametrize("gating", [False, True], ids=["nogate", "gate"])
@pytest.mark.parametrize("k", [1, 5, 32])
@pytest.mark.parametrize("B", [1, 127, 128, 129])
@pytest.mark.parametrize("n_old", [1, 63, 64, 65, 200])
def test_append_equals_batch(dev, n_old, B, k, gating):
    run_case(dev, n_old, B, k, gating, seed=n_old * 1000 + B)


@pytest.mark.parametrize("k", [5, 32])
def test_append_wide_window_runs_several_column_splits(dev, k):
    """B = 1024 new columns: the old rows' window is scanned in two 512-column splits."""
    run_case(dev, 64, 1024, k, True, seed=7)


def test_append_scalar_k_tail(dev):
    """D = 772: D % 16 != 0, the staging's scalar tail of the last k step."""
    run_case(dev, 65, 129, 5, True, D=772, seed=8)


def test_first_append_is_the_batch_call(dev):
    """n_old = 0: the three outputs are empty and the state is knn_gate's."""
    inserted, _, _ = run_case(dev, 0, 130, 5, True, seed=9)
    assert inserted.shape == (0,)


def test_short_rows_fill_and_masked_rows_stay(dev):
    """A row whose list is short before and full after; and with one new keyframe, the rows
    inside its time band see only masked columns and come back untouched."""
    inserted, bcount, acount = run_case(dev, 64, 128, 5, True, seed=10)
    assert np.any((bcount[:64] < 5) & (acount[:64] == 5))
    assert np.any(inserted > 0)
    inserted, _, _ = run_case(dev, 64, 1, 5, True, seed=10)
    band = int(MIN_GAP / 0.765)               # keyframes 64 - band .. 63 are within min_gap of 64
    assert band == 13 and np.all(inserted[64 - band:] == 0)


def stream(dev, dev_in, n, chunks, k, thr, gating, check):
    st = new_state(dev, n, 64, k, thr, gating)
    outs, p = [], 0
    for c in chunks:
        outs.append(st.append(*(x[p:p + c] for x in dev_in)))
        p += c
        if check:
            assert_state_is_batch(st, dev_in, thr, gating)
    assert p == n
    return st, outs


@pytest.mark.parametrize("seed", [1, 2, None], ids=["chunks1", "chunks2", "ones"])
def test_chunk_invariance(dev, seed):
    """N = 300 streamed in seeded random chunkings (sizes 1..97) and in chunks of 1 throughout:
    after every append the state equals knn_gate on the prefix."""
    n, k = 300, 5
    desc, t, floor, has, thr = make_inputs(n, 64, 11)
    dev_in = to_dev(dev, desc, t, floor, has)
    if seed is None:
        chunks = [1] * n
    else:
        rng, chunks = np.random.default_rng(seed), []
        while sum(chunks) < n:
            chunks.append(min(int(rng.integers(1, 98)), n - sum(chunks)))
    stream(dev, dev_in, n, chunks, k, thr, True, check=True)


def test_repeated_runs_give_the_same_bits(dev):
    n, k = 300, 32
    desc, t, floor, has, thr = make_inputs(n, 64, 12)
    dev_in = to_dev(dev, desc, t, floor, has)
    chunks = [70, 1, 129, 100]
    runs = []
    for _ in range(3):
        st, outs = stream(dev, dev_in, n, chunks, k, thr, True, check=False)
        runs.append(snapshot(st) + [x for o in outs for x in o])
    for other in runs[1:]:
        assert len(other) == len(runs[0])
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


def test_the_two_phases_alone_add_up_to_the_call(dev):
    """knn_append(phases=1) then (phases=2) -- the measurement access of the bench tool --
    leaves the state the whole call leaves."""
    from mlgate import _native
    n_old, n, k = 130, 200, 5
    desc, t, floor, has, thr = make_inputs(n, 64, 14)
    dev_in = to_dev(dev, desc, t, floor, has)
    whole, _ = stream(dev, dev_in, n, [n_old, n - n_old], k, thr, True, check=False)
    st = new_state(dev, n, 64, k, thr, True)
    st.append(*(x[:n_old] for x in dev_in))
    st.xn[n_old:n] = whole.xn[n_old:n]
    for dst, src in ((st.t, dev_in[1]), (st.floor, dev_in[2]), (st.has_floor, dev_in[3])):
        dst[n_old:n] = src[n_old:n]
    outs = [_native.ops().knn_append(st.xn, st.t, st.floor, st.has_floor, st.idx, st.sim, st.valid, st.count, n_old, n,
                                     MIN_GAP, thr, k, True, phases) for phases in (1, 2)]
    for a, b in zip(snapshot(st), snapshot(whole)):
        assert torch.equal(a, b)
    assert int(outs[0][0].sum()) > 0


def test_streaming_knn_misuse_raises(dev):
    with pytest.raises(ValueError):
        retrieval.StreamingKnn(8, 64, 33, MIN_GAP, 0.1, True, device=dev)
    with pytest.raises(ValueError):
        retrieval.StreamingKnn(8, 6, 5, MIN_GAP, 0.1, True, device=dev)
    desc, t, floor, has, thr = make_inputs(9, 64, 13)
    d, tt, f, h = to_dev(dev, desc, t, floor, has)
    st = retrieval.StreamingKnn(8, 64, 5, MIN_GAP, thr, True, device=dev)
    with pytest.raises(ValueError):
        st.append(d[:4], tt[:3], f[:4], h[:4])
    with pytest.raises(ValueError):
        st.append(d[:4], tt[:4], f[:5], h[:4])
    with pytest.raises(ValueError):
        st.append(d, tt, f, h)               # 9 keyframes into a capacity of 8
    assert st.n == 0
    st.append(d[:8], tt[:8], f[:8], h[:8])
    with pytest.raises(ValueError):
        st.append(d[8:], tt[8:], f[8:], h[8:])
