"""mlgate.StreamingGate against DeviceGate on the fixture sequence (tests/golden/gate_chain.npz,
40 keyframes): after any chunking of the appends the streamed gate IS the batch gate on the
keyframes seen -- retrieval lists bit for bit, every per-pair match count, inlier count and
decision, every count -- and no ordered pair goes through RANSAC twice.  Exact throughout."""
import numpy as np
import pytest
import torch

import mlgate
from mlgate import retrieval, synthetic
from mlgate.pipeline import DeviceGate, FullSemanticGate, StreamingGate
from oracle import geometry as ogeo

pytestmark = pytest.mark.gpu
CFG = {"A": (True, True), "C": (False, False)}          # tests/test_pipeline_gpu.py's A and C
CHUNKINGS = {"whole": (40,), "mixed": (7, 1, 12, 20), "singles": (1,) * 8 + (32,)}


@pytest.fixture(scope="module")
def chain(golden_dir, dev):
    g = dict(np.load(f"{golden_dir}/gate_chain.npz"))
    n, places, seed, k = (int(x) for x in g["params"])
    seq = synthetic.make_sequence(n, places, seed, tuple((int(f), float(p)) for f, p in g["plan"]))
    thr, gap = (float(x) for x in g["thr_gap"])
    return {"n": n, "k": k, "thr": thr, "gap": gap, "t": np.asarray(seq.t, np.float64), "labels": g["labels"],
            "frames": torch.from_numpy(synthetic.frames_host(seq)).to(dev)}


def common(chain, rg, vg, **kw):
    return dict(k=chain["k"], similarity_threshold=chain["thr"], min_time_gap=chain["gap"],
                retrieval_floor_gating=rg, verifier_floor_gating=vg, K=ogeo.ISEC_K, vit_batch=64, lg_chunk=64, **kw)


def batch_gate(dev, chain, labels, rg, vg, **kw):
    g = DeviceGate(chain["frames"], chain["t"], labels, device=str(dev), record=True, **common(chain, rg, vg, **kw))
    return g, g.step()


@pytest.fixture(scope="module")
def batches(dev, chain):
    return {c: batch_gate(dev, chain, chain["labels"], *CFG[c]) for c in CFG}


def stream(dev, chain, labels, rg, vg, chunks, capacity=None, **kw):
    sg = StreamingGate(capacity or chain["n"], device=str(dev), **common(chain, rg, vg, **kw))
    outs, p = [], 0
    for c in chunks:
        outs.append(sg.append(chain["frames"][p:p + c], chain["t"][p:p + c], labels[p:p + c]))
        p += c
    return sg, outs


def pairs(d):
    return set(zip(d["a"].tolist(), d["b"].tolist()))


def assert_lists_equal(sg, h_idx, h_sim, h_valid, h_count):
    idx, sim, valid, count = (x.cpu().numpy() for x in sg.lists())
    assert np.array_equal(count, h_count)
    live = np.arange(idx.shape[1])[None, :] < count[:, None]
    assert np.array_equal(idx[live], h_idx[live]) and np.array_equal(valid[live], h_valid[live])
    assert np.array_equal(sim[live].view(np.int32), h_sim[live].view(np.int32))


@pytest.mark.parametrize("chunking", list(CHUNKINGS))
@pytest.mark.parametrize("cfg", list(CFG))
def test_streamed_gate_is_the_batch_gate(dev, chain, batches, cfg, chunking):
    g, want = batches[cfg]
    sg, outs = stream(dev, chain, chain["labels"], *CFG[cfg], CHUNKINGS[chunking])
    rep = sg.report()
    assert set(rep) == set(want) - {"pairs_matched_lightglue"}
    assert rep == {key: want[key] for key in rep}
    assert {key: outs[-1][key] for key in rep} == rep
    assert_lists_equal(sg, *g.last_retrieval)
    # every verified ordered pair: the batch's match count, inlier count and decision
    pr, br = sg.pair_results(), g.last_pair_results
    o = np.lexsort((br["b"], br["a"]))
    assert len(pr["a"]) == want["pairs_verified"] > 0
    for key in ("a", "b", "matches", "inliers", "is_valid"):
        assert np.array_equal(pr[key], br[key][o]), key
    # closures announced minus closures retracted = the batch's accepted pairs
    lab = np.asarray(chain["labels"], np.float64)
    acc = br["is_valid"] & ~(np.abs(lab[br["a"]] - lab[br["b"]]) > 0)
    live = set()
    for out in outs:
        gone = pairs(out["retracted"])
        assert gone <= live
        live -= gone
        new = pairs(out["new_closures"])
        assert not (new & live) and len(new) == len(out["new_closures"]["a"])
        live |= new
        assert out["new_closures"]["pose"].shape == (len(new), 4, 4)
    assert live == set(zip(br["a"][acc].tolist(), br["b"][acc].tolist())) and len(live) == want["accepted"]
    assert sum(o_["appended"] for o_ in outs) == chain["n"]


@pytest.mark.parametrize("cfg", list(CFG))
def test_no_ordered_pair_goes_through_ransac_twice(dev, chain, cfg):
    sg = StreamingGate(chain["n"], device=str(dev), **common(chain, *CFG[cfg]))
    seen, total, p = set(), 0, 0
    for c in CHUNKINGS["mixed"]:
        out = sg.append(chain["frames"][p:p + c], chain["t"][p:p + c], chain["labels"][p:p + c])
        p += c
        va, vb = sg.last_append["verified"]
        now = set(zip(va.tolist(), vb.tolist()))
        assert len(now) == len(va) == out["new_pairs_verified"] and not (now & seen)
        seen |= now
        total += len(va)
    assert sg.ransac_pairs == len(seen) == total > 0
    # evicted pairs were verified once and are gone: the live ones are no more than the distinct ones
    assert sg.report()["pairs_verified"] <= len(seen)


def test_retrieval_equality_after_each_single_frame_append(dev, chain, batches):
    """verify=False, one keyframe per append: after each of the 40 appends the lists equal
    knn_gate on the prefix of the batch gate's descriptors (DeviceGate's own retrieval call; its
    ViT descriptors do not depend on the batch a frame is in)."""
    g, _ = batches["A"]
    sg = StreamingGate(chain["n"], device=str(dev), **common(chain, True, True, verify=False))
    for p in range(chain["n"]):
        out = sg.append(chain["frames"][p:p + 1], chain["t"][p:p + 1], chain["labels"][p:p + 1])
        n = p + 1
        ref = retrieval.knn_gate(g.gather.out[:n].contiguous(), g.t_all[:n], g.f_all[:n], g.hf_all[:n], chain["gap"],
                                 chain["thr"], chain["k"], True)
        assert_lists_equal(sg, *(x.cpu().numpy() for x in ref))
        assert out["pairs_verified"] == 0 and out["new_pairs_verified"] == 0 and sg.ransac_pairs == 0
    assert sg.report()["matches"] == batches["A"][1]["matches"]


@pytest.mark.parametrize("rg,vg", [(True, True), (False, True), (False, False)])
def test_float_and_missing_labels_give_the_batch_counts(dev, chain, rg, vg):
    """The labels of test_device_gate_float_and_missing_labels (a NaN, non-integer floors) and a
    None: the incremental floor codes and the NaN-never-rejects gate term give DeviceGate's counts."""
    lab = np.array([float(x) for x in chain["labels"]], np.float64)
    lab[3] = np.nan
    lab[lab == lab[0]] += 0.5
    lab = np.array(lab.tolist(), object)
    lab[11] = None
    _, want = batch_gate(dev, chain, lab, rg, vg)
    sg, _ = stream(dev, chain, lab, rg, vg, CHUNKINGS["mixed"])
    rep = sg.report()
    assert rep == {key: want[key] for key in rep}


def test_pose_is_the_full_gate_pose(dev, chain):
    """new_closures' pose against FullSemanticGate's MatchResult.relative_pose of the same ordered
    pair: both reach k_recover_pose on the same inliers."""
    fg = FullSemanticGate(device=str(dev), k=chain["k"], similarity_threshold=chain["thr"], min_time_gap=chain["gap"],
                          retrieval_floor_gating=True, verifier_floor_gating=True)
    rep = fg.run(chain["frames"], chain["t"], K=ogeo.ISEC_K, floor_labels=chain["labels"])
    ref = {(m.query_idx, m.match_idx): r.relative_pose for m, r in zip(rep.verified, rep.results)}
    sg, outs = stream(dev, chain, chain["labels"], True, True, CHUNKINGS["mixed"])
    worst, seen = 0.0, 0
    for out in outs:
        c = out["new_closures"]
        for a, b, pose in zip(c["a"].tolist(), c["b"].tolist(), c["pose"]):
            assert ref[(a, b)] is not None, (a, b)
            worst = max(worst, float(np.max(np.abs(pose - ref[(a, b)]))))
            seen += 1
    print(f"pose: {seen} accepted pairs, largest |difference| to FullSemanticGate {worst:.3e}")
    assert seen > 0 and worst == 0.0


def test_misuse_raises_before_any_launch(dev, chain):
    assert mlgate.StreamingGate is StreamingGate
    with pytest.raises(ValueError):
        StreamingGate(8, device=str(dev), k=33)
    sg = StreamingGate(4, device=str(dev), **common(chain, True, True, verify=False))
    f, t, lab = chain["frames"], chain["t"], chain["labels"]
    with pytest.raises(ValueError):
        sg.append(f[:5], t[:5], lab[:5])                     # beyond the capacity
    with pytest.raises(ValueError):
        sg.append(f[:2], t[:3], lab[:2])
    assert sg.n == 0
    sg.append(f[:2], t[:2], lab[:2])
    with pytest.raises(ValueError):
        sg.append(f[2:4, :, :-8].contiguous(), t[2:4], lab[2:4])    # another frame size
    with pytest.raises(ValueError):
        sg.append(f[2:5], t[2:5], lab[2:5])
    assert sg.n == 2 and sg.report()["matches"] == 0
