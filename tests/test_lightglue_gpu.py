"""LightGlue on the GPU (lightglue.hip via mlg_lightglue) against the torch-fp32
restatement (oracle/lightglue.py) with the same seeded weights and inputs.

The oracle rounds GEMM / attention operands to bf16 like the kernels, so the two
differ by summation order and the online-softmax normalisation only.  Matches are
discrete decisions (mutual argmax, threshold 0.1, early stop / pruning thresholds),
so the bar is: >= 95 % of matches identical, scores of common matches within 5e-2
absolute, the same number of layers run.  Batched and single-pair calls must agree
bit for bit.  Parity vs the trained LightGlue model is unpinned (offline).
"""
import numpy as np
import pytest
import torch

from mlgate.lightglue import LightGlueGPU
from mlgate.weights import lightglue_state_dict
from oracle.lightglue import Oracle

pytestmark = pytest.mark.gpu


def feats(rng, m, n, overlap=0.6):
    k0 = np.stack([rng.uniform(0, 640, m), rng.uniform(0, 480, m)], 1).astype(np.float32)
    d0 = rng.standard_normal((m, 256)).astype(np.float32)
    d0 /= np.linalg.norm(d0, axis=1, keepdims=True)
    no = int(overlap * min(m, n))
    k1 = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1).astype(np.float32)
    d1 = rng.standard_normal((n, 256)).astype(np.float32)
    k1[:no] = k0[:no] + rng.normal(0, 2, (no, 2)) + np.array([15, -8])
    d1[:no] = d0[:no] + 0.02 * rng.standard_normal((no, 256))
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True) + 1e-12
    return k0, d0, k1.astype(np.float32), d1.astype(np.float32)


@pytest.fixture(scope="module")
def sd():
    return lightglue_state_dict(0)


@pytest.fixture(scope="module")
def lg(dev, sd):
    return LightGlueGPU(sd, device=str(dev))


def _run_gpu(lg, cases):
    kmax = max(max(len(c[0]), len(c[2])) for c in cases)
    F = 2 * len(cases)
    kp = torch.zeros(F, kmax, 2)
    ds = torch.zeros(F, kmax, 256)
    counts = []
    for i, (k0, d0, k1, d1) in enumerate(cases):
        for j, (k, d) in enumerate(((k0, d0), (k1, d1))):
            kp[2 * i + j, :len(k)] = torch.from_numpy(k)
            ds[2 * i + j, :len(k)] = torch.from_numpy(d)
            counts.append(len(k))
    m, s, n, stop = lg.match_device(kp.to(lg.device), ds.to(lg.device), counts, np.arange(0, F, 2),
                                    np.arange(1, F, 2))
    m, s, n = m.cpu().numpy(), s.cpu().numpy(), n.cpu().numpy()
    return [(m[p, :n[p]], s[p, :n[p]], int(stop[p])) for p in range(len(cases))]


@pytest.mark.parametrize("m,n", [(700, 650), (2048, 1900), (1700, 300), (64, 70)])
def test_lightglue_matches_oracle(lg, sd, m, n):
    rng = np.random.default_rng(m + n)
    case = feats(rng, m, n)
    got_m, got_s, got_stop = _run_gpu(lg, [case])[0]
    ref = Oracle(sd).match(*case)
    if got_stop != ref["stop"]:
        # only where the oracle's own early-stop test is within 5e-3 of flipping: then
        # compare against the oracle stopped where the kernel stopped
        lo, hi = ref["depth_band"][min(got_stop, ref["stop"]) - 1]
        assert lo <= 0.95 < hi, (got_stop, ref["stop"], lo, hi)
        ref = Oracle(sd).match(*case, force_stop=got_stop)
    rm, rs = ref["matches"].numpy(), ref["scores"].numpy()
    assert got_stop == ref["stop"]
    g = {tuple(x): i for i, x in enumerate(got_m.tolist())}
    r = {tuple(x): i for i, x in enumerate(rm.tolist())}
    common = set(g) & set(r)
    assert len(common) >= 0.95 * max(len(g), len(r)), (len(common), len(g), len(r))
    gi = np.array([g[c] for c in common], int)
    ri = np.array([r[c] for c in common], int)
    np.testing.assert_allclose(got_s[gi], rs[ri], atol=5e-2)
    assert np.all(np.diff(got_m[:, 0]) > 0)  # ascending image0 index, as torch.where


def test_lightglue_batched_equals_single(lg):
    rng = np.random.default_rng(3)
    cases = [feats(rng, 300, 280), feats(rng, 1600, 1550), feats(rng, 40, 90), feats(rng, 800, 10)]
    batch = _run_gpu(lg, cases)
    for c, b in zip(cases, batch):
        s = _run_gpu(lg, [c])[0]
        assert np.array_equal(s[0], b[0]) and np.array_equal(s[1], b[1]) and s[2] == b[2]


def test_lightglue_empty_side(lg):
    rng = np.random.default_rng(4)
    k0, d0, k1, d1 = feats(rng, 50, 40)
    res = _run_gpu(lg, [(k0, d0, k1[:0], d1[:0]), (k0, d0, k1, d1)])
    assert len(res[0][0]) == 0
    assert len(res[1][0]) > 0


def test_lightglue_against_fp32_reference(dev, lg, sd):
    """The GPU matcher (bf16 GEMM / attention operands) against the reference's arithmetic
    -- the fp32 forward without bf16 emulation -- on SuperPoint features of a synthetic
    revisit pair (true correspondences): match sets overlap >= 99 %, scores of common
    matches within 5e-2."""
    from mlgate import synthetic
    from mlgate.superpoint import SuperPointGPU
    seq = synthetic.make_sequence(40, 4, 2)
    same = [i for i in range(1, 40) if seq.place_of[i] == seq.place_of[0]]
    fr = torch.from_numpy(synthetic.frames_host(seq, [0, same[0]])).to(dev)
    f0, f1 = SuperPointGPU(device=str(dev)).extract(list(fr.cpu().numpy()))
    case = (f0["keypoints"], f0["descriptors"], f1["keypoints"], f1["descriptors"])
    gm, gs, gstop = _run_gpu(lg, [case])[0]
    ref = Oracle(sd, emulate_bf16=False).match(*case)
    g = {tuple(x): i for i, x in enumerate(gm.tolist())}
    r = {tuple(x): i for i, x in enumerate(ref["matches"].numpy().tolist())}
    common = set(g) & set(r)
    overlap = len(common) / max(len(g), len(r), 1)
    print(f"fp32 LightGlue: {len(g)} vs {len(r)} matches, overlap {overlap:.4f}, stop {gstop} vs {ref['stop']}")
    assert len(r) > 100 and overlap >= 0.99  # measured 0.9976 (profiles/r03ae_tolerances.log)
    gi = np.array([g[c] for c in common])
    ri = np.array([r[c] for c in common])
    np.testing.assert_allclose(gs[gi], ref["scores"].numpy()[ri], atol=5e-2)


def test_lightglue_repeated_frames_equal_single_pairs(lg):
    """Frames shared by several pairs of one call run layer 0's self block once per frame
    (csrc/lightglue.hip frame layout): every pair's matches, scores and stop layer must be
    bit-identical to matching that pair alone."""
    rng = np.random.default_rng(21)
    sizes = [600, 1200, 450, 900]
    frames = []
    for m in sizes:
        k = np.stack([rng.uniform(0, 640, m), rng.uniform(0, 480, m)], 1).astype(np.float32)
        d = rng.standard_normal((m, 256)).astype(np.float32)
        frames.append((k, d / np.linalg.norm(d, axis=1, keepdims=True)))
    for i in (1, 3):  # overlapping views of frame 0
        k0, d0 = frames[0]
        no = min(len(k0), sizes[i]) // 2
        k, d = frames[i]
        k[:no] = k0[:no] + rng.normal(0, 2, (no, 2)).astype(np.float32)
        d[:no] = d0[:no] + 0.02 * rng.standard_normal((no, 256)).astype(np.float32)
        d[:no] /= np.linalg.norm(d[:no], axis=1, keepdims=True)
    kmax = max(sizes)
    kp = torch.zeros(len(frames), kmax, 2)
    ds = torch.zeros(len(frames), kmax, 256)
    for f, (k, d) in enumerate(frames):
        kp[f, :len(k)], ds[f, :len(k)] = torch.from_numpy(k), torch.from_numpy(d)
    kp, ds = kp.to(lg.device), ds.to(lg.device)
    pa, pb = np.array([0, 0, 1, 3, 2, 0], np.int32), np.array([1, 3, 3, 0, 0, 2], np.int32)
    m, s, n, stop = lg.match_device(kp, ds, sizes, pa, pb)
    m, s, n = m.cpu().numpy(), s.cpu().numpy(), n.cpu().numpy()
    for p in range(len(pa)):
        m1, s1, n1, st1 = lg.match_device(kp, ds, sizes, pa[p:p + 1], pb[p:p + 1])
        k1 = int(n1[0])
        assert k1 == n[p] and st1[0] == stop[p]
        assert np.array_equal(m1[0, :k1].cpu().numpy(), m[p, :k1]) and np.array_equal(s1[0, :k1].cpu().numpy(), s[p, :k1])
    assert n[0] > 0 and n[3] > 0


def test_lightglue_swapped_pair_is_the_exact_swap(lg):
    """LightGlue(b, a) == swap(LightGlue(a, b)) bit for bit -- matches (re-sorted by the new
    image0 index), scores and stop layers -- so the full gate's once-per-unordered-pair
    matching (pipeline.py) gives every ordered pair exactly its own call's result.  Cases
    cover pruning (> 1536 keypoints), early stopping and ragged sizes; frame indices on
    both sides of each other (the assignment's canonical cross-term order, lightglue.hip
    k_asg_sim)."""
    rng = np.random.default_rng(31)
    cases = [feats(rng, 2048, 1900), feats(rng, 1700, 300), feats(rng, 700, 650), feats(rng, 64, 70),
             feats(rng, 1200, 1250, overlap=0.9), feats(rng, 900, 880, overlap=0.1)]
    kmax = 2048
    F = 2 * len(cases)
    kp = torch.zeros(F, kmax, 2)
    ds = torch.zeros(F, kmax, 256)
    counts = []
    for i, (k0, d0, k1, d1) in enumerate(cases):
        for j, (k, d) in enumerate(((k0, d0), (k1, d1))):
            kp[2 * i + j, :len(k)] = torch.from_numpy(k)
            ds[2 * i + j, :len(k)] = torch.from_numpy(d)
            counts.append(len(k))
    kp, ds = kp.to(lg.device), ds.to(lg.device)
    a, b = np.arange(0, F, 2, dtype=np.int32), np.arange(1, F, 2, dtype=np.int32)
    m1, s1, n1, st1 = (x.cpu().numpy() if torch.is_tensor(x) else x for x in lg.match_device(kp, ds, counts, a, b))
    m2, s2, n2, st2 = (x.cpu().numpy() if torch.is_tensor(x) else x for x in lg.match_device(kp, ds, counts, b, a))
    assert np.array_equal(st1, st2)
    assert np.array_equal(n1, n2)
    for p in range(len(cases)):
        k = int(n1[p])
        o = np.argsort(m1[p, :k, 1])
        assert np.array_equal(m2[p, :k, 0], m1[p, :k, 1][o]) and np.array_equal(m2[p, :k, 1], m1[p, :k, 0][o]), p
        assert np.array_equal(s2[p, :k].view(np.uint32), s1[p, :k][o].view(np.uint32)), p
    assert n1.min() > 0


def test_lightglue_no_early_stop_prunes_on_matchability_only(dev, sd):
    """depth_confidence <= 0 (early stopping off): upstream computes no token confidences,
    so a point is kept iff its matchability > 1 - width_confidence (get_pruning_mask with
    confidences None); the kernel's keep bit must drop the confidence term too."""
    lg = LightGlueGPU(sd, device=str(dev), depth_confidence=-1)
    rng = np.random.default_rng(77)
    case = feats(rng, 2048, 1900)
    got_m, got_s, got_stop = _run_gpu(lg, [case])[0]
    ref = Oracle(sd).match(*case, depth_confidence=-1)
    assert got_stop == ref["stop"] == 9
    rm, rs = ref["matches"].numpy(), ref["scores"].numpy()
    g = {tuple(x): i for i, x in enumerate(got_m.tolist())}
    r = {tuple(x): i for i, x in enumerate(rm.tolist())}
    common = set(g) & set(r)
    assert len(common) >= 0.95 * max(len(g), len(r)), (len(common), len(g), len(r))


def test_malformed_weight_list_is_refused(dev, lg):
    """The lightglue op checks every tensor of its list before launching (weight_tables.h)."""
    from mlgate import _native
    from weight_corruptions import assert_refused
    kp, ds = torch.zeros(2, 8, 2, device=dev), torch.zeros(2, 8, 256, device=dev)
    host = lambda a: torch.tensor(a, dtype=torch.int32)  # noqa: E731
    assert_refused(lambda b: _native.ops().lightglue(kp, ds, host([8, 8]), host([0]), host([1]), b, 0.95, 0.99, 0.1,
                                                     1536), lg._w, 35, "self[3].Wf1")
