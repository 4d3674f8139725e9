"""The re-ranking stage in the frame-sharded gate: DeviceGate(rerank_top_k=2) with world 2 on
cuda:0 over gloo (collectives staged through host copies, the code path RCCL runs on device
tensors), the bank of local features all-gathered through the second RowGather.  The
re-ranked lists of both ranks' query rows, in rank order, the all-reduced counts and every
ordered pair's (matches, inliers, is_valid) equal the world-1 run exactly."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _case():
    from mlgate import synthetic
    from oracle import geometry as ogeo
    g = np.load(os.path.join(ROOT, "tests", "golden", "gate_chain.npz"))
    n, places, seed, _ = (int(x) for x in g["params"])
    seq = synthetic.make_sequence(n, places, seed, tuple((int(f), float(p)) for f, p in g["plan"]))
    kw = dict(k=5, similarity_threshold=-1.0, min_time_gap=float(g["thr_gap"][1]), retrieval_floor_gating=False,
              vit_batch=64, lg_chunk=64, rerank_top_k=2, record=True)
    return seq, np.asarray(g["labels"]), kw, ogeo.ISEC_K


def _lists(gate):
    """The re-ranked lists as plain data: per query row its kept (idx, sim bits, cross bits, score bits)."""
    r_idx, r_sim, r_cross, r_score, r_count = gate.last_rerank
    return [[(int(r_idx[i, s]), int(r_sim[i, s:s + 1].view(np.uint32)[0]), int(r_cross[i, s:s + 1].view(np.uint32)[0]),
              int(r_score[i, s:s + 1].view(np.uint64)[0])) for s in range(int(r_count[i]))]
            for i in range(len(r_count))]


def _pairs(gate):
    r = gate.last_pair_results
    return {(int(a), int(b)): (int(n), int(i), bool(v))
            for a, b, n, i, v in zip(r["a"], r["b"], r["matches"], r["inliers"], r["is_valid"])}


def _worker(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mlgate import distributed as mdist
    from mlgate import synthetic
    from mlgate.pipeline import DeviceGate
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    seq, labels, kw, K = _case()
    lo, hi = mdist.shard(seq.n, world, rank)
    frames = torch.from_numpy(synthetic.frames_host(seq, np.arange(lo, hi))).to(dev)
    g = DeviceGate(frames, seq.t, labels, world, rank, dev, K=K, **kw)
    out = g.step()
    out.pop("features_exchanged_bytes", 0)
    keys = sorted(out)
    tot = torch.tensor([out[k_] for k_ in keys], dtype=torch.int64)
    dist.all_reduce(tot)
    parts = mdist.gather_objects_to_rank0((_lists(g), _pairs(g)), world, rank)
    if rank == 0:
        g1 = DeviceGate(torch.from_numpy(synthetic.frames_host(seq)).to(dev), seq.t, labels, 1, 0, dev, K=K, **kw)
        o1 = g1.step()
        merged, dup = {}, 0
        for _, p in parts:
            dup += len(set(p) & set(merged))
            merged.update(p)
        ref = _pairs(g1)
        res = {"counts_w": dict(zip(keys, tot.tolist())), "counts_w1": {k_: o1[k_] for k_ in keys},
               "same_lists": sum((l for l, _ in parts), []) == _lists(g1), "dup": dup, "same_pairs": merged == ref,
               "differing": [str(p) for p in ref if merged.get(p) != ref[p]][:10], "pairs": len(ref),
               "reranked_out": o1["reranked_out"]}
        with open(out_path, "w") as f:
            json.dump(res, f)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_rerank_equals_single_rank(tmp_path):
    out = str(tmp_path / "res.json")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    res = json.load(open(out))
    print(json.dumps(res))
    assert res["same_lists"]
    assert res["counts_w"] == res["counts_w1"]
    assert res["dup"] == 0 and res["same_pairs"], res["differing"]
    assert res["pairs"] > 0 and res["reranked_out"] > 0
