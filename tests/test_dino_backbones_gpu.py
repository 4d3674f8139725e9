"""DINOv2 ViT-S/14 and ViT-L/14 through mlg_dino_forward against the float32 CPU restatement
(tests/dino_restatement.py), and the layers above it: DinoVit, the CricaVPR / AnyLoc drop-ins,
SemanticPlaceRecognition and DeviceGate with a backbone.

The input throughout is three 480 x 640 frames (two rectangle scenes and one noise frame) at
image size 322: M = 1590 token rows = six full 256-row M-tiles and a ragged one of 54 rows,
T = 530 padded to 576.  On ViT-S every split GEMM with a 128-column tail (patch 384, qkv 1152,
proj 384, fc2 384) then runs in both M positions.  Weights are seeded synthetic ones.

Bars: those of tests/test_vit_gpu.py for ViT-B (split forward: descriptor 1 - cos < 1e-9, local
features < 1e-7 per token, pairwise normalised similarities within 1e-6; plain bf16 forward:
1e-4 and 1e-3).  The restatement is not what limits them: against a float64 run of the same
forward it sits at 7e-14 (descriptor) and 1e-12 (local) at all three widths.  Each parity test
prints its measured values before it asserts."""
import functools

import numpy as np
import pytest
import torch

import dino_restatement as R
from mlgate import _native
from mlgate.vit import DinoVit, VitB14, pack_weights
from mlgate.weights import backbone_config, synthetic_state_dict
from weight_corruptions import assert_refused

pytestmark = pytest.mark.gpu

S14, B14, L14 = "dinov2_vits14", "dinov2_vitb14", "dinov2_vitl14"
NEW = [S14, L14]
cosd = torch.nn.functional.cosine_similarity


def scene(rng, h=480, w=640):
    """Rectangles + noise, the synthetic-frame recipe of tests/test_vit_gpu.py."""
    img = np.zeros((h, w, 3), np.uint8)
    for _ in range(30):
        x, y = rng.integers(0, w - 60), rng.integers(0, h - 60)
        ww, hh = rng.integers(20, 120), rng.integers(20, 120)
        img[y:y + hh, x:x + ww] = rng.integers(60, 255, 3)
    return np.clip(img.astype(np.int32) + rng.integers(0, 30, img.shape), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def sd_of(backbone):
    return synthetic_state_dict(0, backbone)


@functools.lru_cache(maxsize=None)
def engine(backbone, precise=True):
    """One packed engine per (backbone, packing); the tests set .max_batch (read at each call)."""
    return DinoVit(sd_of(backbone), backbone=backbone, device="cuda", max_batch=4, precise=precise)


@pytest.fixture(scope="module")
def frames():
    rng = np.random.default_rng(1)
    return np.stack([scene(rng) for _ in range(2)] + [rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)])


@pytest.fixture(scope="module")
def refs(frames):
    """backbone -> the restatement's tokens [3, 529, E] of the three frames at 322 (computed once)."""
    torch.set_num_threads(8)
    x = torch.cat([R.preprocess(f) for f in frames])
    cache = {}

    def get(backbone):
        if backbone not in cache:
            cache[backbone] = R.forward_tokens(x, sd_of(backbone), backbone)
        return cache[backbone]
    return get


def run(eng, x, max_batch, with_local=True):
    eng.max_batch = max_batch
    out = eng.forward(x, with_local=with_local)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("backbone", NEW)
def test_split_forward_matches_the_restatement(dev, frames, refs, backbone):
    """Measured on an MI355X: ViT-S descriptor 3.2e-12, local 5.9e-11, pairwise
    9.1e-8; ViT-L 4.6e-11, 2.1e-10, 5.1e-7 -- inside ViT-B's bars, none adjusted."""
    E = backbone_config(backbone)[0]
    desc, local = run(engine(backbone), torch.from_numpy(frames).to(dev), 4)
    assert desc.shape == (3, E) and local.shape == (3, 528, E) and desc.dtype == local.dtype == torch.float32
    desc, local = desc.cpu().double(), local.cpu().double()
    tok = refs(backbone)
    ref_d = R.gem(tok).double()
    dcos = [1 - cosd(desc[b], ref_d[b], dim=0).item() for b in range(3)]
    lcos = [(1 - cosd(local[b], R.local(tok)[b].double(), dim=1)).max().item() for b in range(3)]
    nrm = lambda X: X / X.norm(dim=1, keepdim=True)  # noqa: E731
    pair = (nrm(desc) @ nrm(desc).T - nrm(ref_d) @ nrm(ref_d).T).abs().max().item()
    print(f"{backbone} split: descriptor 1-cos {max(dcos):.3e}, local 1-cos {max(lcos):.3e}, pairwise {pair:.3e}")
    assert max(dcos) < 1e-9, dcos
    assert max(lcos) < 1e-7, lcos
    assert pair < 1e-6


@pytest.mark.parametrize("backbone", NEW)
def test_plain_bf16_forward_matches_the_restatement(dev, frames, refs, backbone):
    desc, local = run(engine(backbone, False), torch.from_numpy(frames).to(dev), 4)
    desc, local = desc.cpu().double(), local.cpu().double()
    tok = refs(backbone)
    ref_d = R.gem(tok).double()
    dcos = [1 - cosd(desc[b], ref_d[b], dim=0).item() for b in range(3)]
    lcos = [(1 - cosd(local[b], R.local(tok)[b].double(), dim=1)).max().item() for b in range(3)]
    print(f"{backbone} bf16: descriptor 1-cos {max(dcos):.3e}, local 1-cos {max(lcos):.3e}")
    assert max(dcos) < 1e-4, dcos
    assert max(lcos) < 1e-3, lcos


def test_anyloc_flags_at_518_vits(dev, frames):
    """AnyLoc's call: one frame at 518, mean pooling, channels kept (T = 1370: a ragged M-tile of 90)."""
    torch.set_num_threads(8)
    eng = DinoVit(sd_of(S14), backbone=S14, device="cuda", image_size=518, max_batch=1, pool="mean", swap_rb=False)
    desc = eng.forward(torch.from_numpy(frames[:1]).to(dev))
    torch.cuda.synchronize()
    ref = R.mean_pool(R.forward_tokens(R.preprocess(frames[0], 518, swap_rb=False), sd_of(S14), S14))[0]
    err = 1 - cosd(desc[0].cpu().double(), ref.double(), dim=0).item()
    print(f"AnyLoc flags, ViT-S at 518: descriptor 1-cos {err:.3e}")
    assert desc.shape == (1, 384) and err < 1e-9, err


@pytest.mark.parametrize("backbone", NEW)
def test_split_forward_does_not_depend_on_the_batching(dev, frames, backbone):
    x = torch.from_numpy(frames).to(dev)
    d2, l2 = run(engine(backbone), x, 2)
    d3, l3 = run(engine(backbone), x, 3)
    assert torch.equal(d2, d3) and torch.equal(l2, l3)


@pytest.mark.parametrize("backbone,reps", [(S14, 21), (L14, 11)])
def test_split_forward_walking_tiles(dev, frames, backbone, reps):
    """More output tiles than CUs even in the narrowest GEMM (proj: 2 N-tiles at ViT-S, its second
    half padding; 4 at ViT-L), so every persistent split GEMM walks to a second tile."""
    x = torch.from_numpy(np.tile(frames, (reps, 1, 1, 1))).to(dev)
    eng = engine(backbone)
    n_tiles = (backbone_config(backbone)[0] + 255) // 256
    m_tiles = (len(x) * (eng.n_patches + 1) + 255) // 256
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert m_tiles * n_tiles > cus, (m_tiles, n_tiles, cus)
    big = run(eng, x, len(x), with_local=False)
    small = run(eng, x, 4, with_local=False)
    assert torch.equal(big, small)


@pytest.mark.parametrize("precise", [True, False])
def test_vitb_through_the_new_entry_point_is_vitb14(dev, frames, precise):
    x = torch.from_numpy(frames).to(dev)
    new = DinoVit(sd_of(B14), backbone=B14, device="cuda", max_batch=2, precise=precise)
    old = VitB14(sd_of(B14), device="cuda", max_batch=2, precise=precise)
    dn, ln = new.forward(x, with_local=True)
    do, lo = old.forward(x, with_local=True)
    torch.cuda.synchronize()
    assert dn.shape == (3, 768) and torch.equal(dn, do) and torch.equal(ln, lo)


def test_malformed_weight_lists_are_refused(dev):
    ops = _native.ops()
    x = torch.zeros(1, 32, 32, 3, dtype=torch.uint8, device=dev)
    d384, d1024 = torch.empty(1, 384, device=dev), torch.empty(1, 1024, device=dev)
    with pytest.raises(RuntimeError, match=r"dino weights\[0\] \(patch_w\)"):
        ops.dino_forward_into(x, pack_weights(sd_of(B14), dev, 23, True), 384, 322, 4, 2, d384, None)
    ws, wl = engine(S14)._w, engine(L14)._w
    with pytest.raises(RuntimeError, match=f"expected {len(wl)} tensors, got {len(wl) - 14}"):
        ops.dino_forward_into(x, wl[:4 + 23 * 14] + wl[-2:], 1024, 322, 4, 2, d1024, None)
    assert_refused(lambda b: ops.dino_forward_into(x, b, 384, 322, 4, 2, d384, None), ws, 6, "blocks[0].qkv_w")
    assert_refused(lambda b: ops.dino_forward_into(x, b, 1024, 322, 4, 2, d1024, None), wl, 4 + 23 * 14 + 11,
                   "blocks[23].fc2_w")
    with pytest.raises(RuntimeError, match=r"desc must be \[B, 384\]"):
        ops.dino_forward_into(x, ws, 384, 322, 4, 2, d1024, None)
    with pytest.raises(RuntimeError, match="embed must be 384"):
        ops.dino_forward_into(x, ws, 512, 322, 4, 2, d384, None)


# ---------------------------------------------------------------------- the drop-in
def test_cricavpr_dropin_vits(dev, frames, refs, monkeypatch):
    from mlgate.vpr import CricaVPR
    from oracle import xcorr as oxc
    for var in ("MLGATE_DINOV2_WEIGHTS", "MLGATE_CRICAVPR_NATIVE"):
        monkeypatch.delenv(var, raising=False)
    m = CricaVPR(backbone=S14, descriptor_dim=384, device="cuda")
    with pytest.warns(UserWarning, match="synthetic dinov2_vits14"):
        d = m.extract_descriptor(frames[0])
    assert m.feat_dim == 384 and d.shape == (384,) and d.dtype == np.float32
    tok = refs(S14)
    err = 1 - cosd(torch.from_numpy(d).double(), R.gem(tok)[0].double(), dim=0).item()
    assert err < 1e-9, err
    f0, f1 = m.extract_local_features(frames[0]), m.extract_local_features(frames[1])
    assert f0.shape == f1.shape == (1, 528, 384) and f0.dtype == np.float32
    s = m.compute_cross_correlation_score(f0, f1)
    assert abs(s - oxc.xcorr_score(f0, f1)) < 1e-5, (s, oxc.xcorr_score(f0, f1))


def test_anyloc_dropin_vitl(dev, frames, monkeypatch):
    from mlgate.vpr import AnyLoc
    for var in ("MLGATE_DINOV2_WEIGHTS", "MLGATE_ANYLOC_NATIVE"):
        monkeypatch.delenv(var, raising=False)
    m = AnyLoc(backbone=L14, descriptor_dim=1024, device="cuda")
    with pytest.warns(UserWarning, match="synthetic dinov2_vitl14"):
        d = m.extract_descriptor(frames[0])
    assert m.feat_dim == 1024 and d.shape == (1024,) and d.dtype == np.float32 and np.isfinite(d).all()


def test_semantic_place_recognition_with_vits(dev, monkeypatch):
    """12 frames (6 scenes and their shifted revisits) 20 s apart: find_loop_closures returns what
    oracle.retrieval computes from the same descriptors, and each revisit finds its scene."""
    from mlgate.vpr import CricaVPR, SemanticPlaceRecognition, floor_codes
    from oracle import retrieval as oret
    for var in ("MLGATE_DINOV2_WEIGHTS", "MLGATE_CRICAVPR_NATIVE"):
        monkeypatch.delenv(var, raising=False)
    rng = np.random.default_rng(7)
    scenes = [scene(rng) for _ in range(6)]
    imgs = scenes + [np.roll(s, 12, axis=1) for s in scenes]
    t = [20.0 * i for i in range(12)]
    floors = [0, 0, 0, 1, 1, 1, 0, 0, 1, 1, 1, 0]  # revisits 2 and 5 come back on another floor
    spr = SemanticPlaceRecognition("cricavpr", device="cuda")
    spr.vpr = CricaVPR(backbone=S14, descriptor_dim=384, device="cuda", use_reranking=True)
    with pytest.warns(UserWarning, match="synthetic"):
        spr.add_images(imgs, t, floors)
    X = np.stack([d.descriptor for d in spr.vpr.descriptors])
    assert X.shape == (12, 384) and spr.vpr._feature_cache[11].shape == (1, 528, 384)
    got = spr.find_loop_closures(enable_floor_gating=True, k=3)
    codes, has = floor_codes(floors)
    q, mm, sim, valid = oret.find_loop_closures(X, np.asarray(t), np.asarray(codes), np.asarray(has), 10.0, 0.5, 3, True)
    assert [(g.query_idx, g.match_idx, g.is_valid) for g in got] == [(int(a), int(b), bool(v)) for a, b, v in
                                                                    zip(q, mm, valid)]
    assert np.max(np.abs(np.array([g.similarity for g in got]) - sim)) <= 4e-6
    best = {}
    for g in got:
        best.setdefault(g.query_idx, g.match_idx)
    assert all(best[i + 6] == i for i in range(6)), best
    # the rerank cache works at the width: the batched pass scores [528, 384] features
    rr = spr.vpr.rerank_candidates(6, [(0, 0.9), (1, 0.9)], top_k=2)
    assert rr[0][0] == 0 and rr[0][1] > rr[1][1]


def test_device_gate_with_vits(dev):
    from mlgate import retrieval, synthetic
    from mlgate.pipeline import DeviceGate
    seq = synthetic.make_sequence(24, 6, 3)
    x = torch.from_numpy(synthetic.frames_host(seq)).to(dev)
    labels = np.asarray([i // 8 for i in range(24)])
    g = DeviceGate(x, seq.t, labels, device=str(dev), k=5, similarity_threshold=0.3, min_time_gap=2.0, verify=False,
                   vit_batch=16, record=True, backbone=S14)
    out = g.step()
    torch.cuda.synchronize()
    assert g.gather.out.shape == (24, 384) and g.local_feats.shape == (24, 528, 384)
    ref_d, ref_l = run(engine(S14), x, 16)
    assert torch.equal(g.gather.out, ref_d) and torch.equal(g.local_feats, ref_l)
    idx, sim, valid, count = retrieval.knn_gate(g.gather.out, g.t_all, g.f_all, g.hf_all, 2.0, 0.3, 5, True)
    h_idx, h_sim, h_valid, h_count = g.last_retrieval
    assert np.array_equal(h_count, count.cpu().numpy()) and out["matches"] == int(h_count.sum()) > 0
    live = np.arange(5)[None, :] < h_count[:, None]
    assert np.array_equal(h_idx[live], idx.cpu().numpy()[live]) and np.array_equal(h_valid[live], valid.cpu().numpy()[live])
    assert np.array_equal(h_sim[live], sim.cpu().numpy()[live])
