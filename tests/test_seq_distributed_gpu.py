"""The sequence-consistency stage in the frame-sharded gate: DeviceGate(seq_radius=3) with
world 2 on cuda:0 over gloo (two processes), on the 96-frame walk's descriptors.  Nothing new
is exchanged: each rank judges its own query rows against the gathered descriptors, windows
reaching into the other rank's frames.  The union of the ranks' kept pairs, their per-entry
outputs in rank order and the summed counts equal the world-1 run exactly."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _data(g):
    seq = [a.tobytes().hex() for a in g.last_sequence]
    return seq, list(zip(g.last_pairs[0].tolist(), g.last_pairs[1].tolist()))


def _worker(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import seq_restatement as sr
    from mlgate import distributed as mdist
    from test_seq_gpu import walk_gate
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    kw = dict(seq_radius=sr.W, seq_threshold=sr.SEQ_THR)
    g = walk_gate(dev, world, rank, **kw)
    out = g.step()
    keys = sorted(out)
    tot = torch.tensor([out[k_] for k_ in keys], dtype=torch.int64)
    dist.all_reduce(tot)
    parts = mdist.gather_objects_to_rank0(_data(g), world, rank)
    if rank == 0:
        g1 = walk_gate(dev, **kw)
        o1 = g1.step()
        seq1, pairs1 = _data(g1)
        res = {"counts_w": dict(zip(keys, tot.tolist())), "counts_w1": {k_: o1[k_] for k_ in keys},
               "same_pairs": sum((p for _, p in parts), []) == pairs1, "pairs": len(pairs1),
               "same_outputs": ["".join(s[n] for s, _ in parts) == seq1[n] for n in range(4)]}
        with open(out_path, "w") as f:
            json.dump(res, f)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_sequence_check_equals_single_rank(tmp_path):
    out = str(tmp_path / "res.json")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    res = json.load(open(out))
    print(json.dumps(res))
    assert res["counts_w"] == res["counts_w1"]
    assert res["counts_w1"]["sequence_rejected"] == 12 and res["counts_w1"]["sequence_candidates"] == 158
    assert res["same_pairs"] and res["pairs"] == 146
    assert all(res["same_outputs"])
