"""CricaVPR's native branch on the GPU (csrc/crica.hip, mlgate/crica.py) against the float64
restatement (tests/crica_restatement.py).  Every bar is a reference-side quantity or the
project's bar for the split-bf16 forward: the float32 twin's own error for the pool, 1e-9
(tests/test_vit_gpu.py) for the encoder, 4e-9 end to end; e_f32 and e_split are printed beside
each measured value.  tests/test_crica_cpu.py asserts the fixtures' conditions."""
import copy
import warnings

import numpy as np
import pytest
import torch

import crica_restatement as R
from mlgate import _native
from mlgate.crica import CricaGPU, pack_head
from mlgate.vpr import CricaVPR, SemanticPlaceRecognition

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(dev):
    return CricaGPU(R.e2e_fixture()["state_dict"], device=str(dev), max_batch=64, group=1)


@pytest.fixture(scope="module")
def frames7(dev):
    """7 small frames (the trunk resizes them to 322 x 322): structure plus noise, all different."""
    rng = np.random.default_rng(31)
    yy, xx = np.mgrid[0:96, 0:128]
    out = [np.clip(127 + 80 * (np.sin(xx / (4.0 + 3 * i) + i) * np.cos(yy / (5.0 + 2 * i)))[..., None] +
                   rng.normal(0, 10, (96, 128, 3)), 0, 255) for i in range(7)]
    return torch.from_numpy(np.stack(out).astype(np.uint8)).to(dev)


def _dev(a, dev):
    return torch.tensor(np.asarray(a)).to(dev)  # a copy: the fixtures are read-only


# ------------------------------------------------------------ 1. the pool against float64
@pytest.mark.parametrize("B, g, p", R.POOL_CASES)
def test_pool_matches_float64(dev, B, g, p):
    """Per row of [B, 14, 768] (row 0: the CLS token's LayerNorm), the relative L2 error against
    float64 is at most 8 x the float32 twin's own."""
    x, nw, nb = R.pool_fixture(B, g)
    got = _native.ops().crica_pool(_dev(x, dev), _dev(nw, dev), _dev(nb, dev), p).cpu().numpy()
    assert got.shape == (B, 14, 768) and got.dtype == np.float32 and np.all(np.isfinite(got))
    ref = R.pool(x, nw, nb, p)
    err, floor = R.rel_l2(got, ref), R.rel_l2(R.pool(x, nw, nb, p, "f32"), ref)
    print(f"B {B} g {g} p {p}: rel L2 max {err.max():.3e}, e_f32 max {floor.max():.3e}, "
          f"worst ratio {np.max(err / floor):.2f} (CLS rows {np.max(err[:, 0] / floor[:, 0]):.2f})")
    assert np.all(err <= 8 * floor), (err / floor).round(2)
    assert np.all(got[:, 1:] > 0)


# ------------------------------------------------------------ 2. the encoder against float64
@pytest.mark.parametrize("B, group", R.ENCODER_CASES)
def test_encoder_matches_float64(dev, engine, B, group):
    ref, e_f32, e_split = R.encoder_reference(B, group)
    got = engine.encode(_dev(R.pooled_fixture(B), dev), group).cpu().numpy()
    assert got.shape == (B, R.DIM) and got.dtype == np.float32 and np.all(np.isfinite(got))
    err = max(R.one_minus_cos(a, b) for a, b in zip(got, ref))
    print(f"B {B} group {group}: 1 - cos {err:.3e}, e_split {e_split:.3e}, e_f32 {e_f32:.3e}")
    assert np.all(np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1) <= 1e-5)
    assert err <= 1e-9


# ------------------------------------------------------------ 3. invariance, bit for bit
def test_groups_do_not_depend_on_the_call(dev, engine):
    x = _dev(R.pooled_fixture(7), dev)
    base = engine.encode(x, 3)  # groups {0, 1, 2}, {3, 4, 5}, {6}
    assert torch.equal(engine.encode(x, 3), base)
    assert torch.equal(engine.encode(x[3:6], 3), base[3:6])
    assert torch.equal(engine.encode(x[6:], 3), base[6:])
    assert torch.equal(engine.encode(x[6:], 1), base[6:])  # a short last group of one is a frame alone
    moved = engine.encode(x[[3, 4, 5, 0, 1, 2, 6]].contiguous(), 3)  # the first two groups swapped
    assert torch.equal(moved[:3], base[3:6]) and torch.equal(moved[3:6], base[:3]) and torch.equal(moved[6], base[6])
    assert not torch.equal(engine.encode(x, 1)[:6], base[:6])
    ones = engine.encode(x, 1)
    for b in range(7):
        assert torch.equal(engine.encode(x[b:b + 1], 1)[0], ones[b])


def test_forward_chunks_on_group_boundaries(dev, engine, frames7):
    whole = copy.copy(engine)
    whole.group = 3
    chunked = copy.copy(whole)
    chunked.max_batch = 4  # 3 frames per call
    want = whole.forward(frames7)
    assert tuple(want.shape) == (7, R.DIM)
    assert torch.equal(chunked.forward(frames7), want)
    assert torch.equal(whole.forward(frames7[3:6]), want[3:6])
    singles = engine.forward(frames7[:3])  # group 1: B frames against B single-frame calls
    for b in range(3):
        assert torch.equal(engine.forward(frames7[b:b + 1])[0], singles[b])
    assert torch.equal(engine.forward(frames7[:3]), singles)


# ------------------------------------------------------------ 4. composition
def test_forward_is_trunk_pool_encode(dev, engine, frames7):
    frames = frames7[:4]
    two = copy.copy(engine)
    two.group = 2
    desc, local = two.forward(frames, with_local=True)
    tokens = two.trunk(frames)
    assert tuple(tokens.shape) == (4, 530, 768)
    assert torch.equal(two.encode(two.pool(tokens)), desc)
    assert torch.equal(two.forward(frames), desc)
    gem, want_local = engine._vit.forward(frames, with_local=True)
    assert tuple(local.shape) == (4, 528, 768) and torch.equal(local, want_local)


# ------------------------------------------------------------ 5. end to end
@pytest.mark.parametrize("group", [1, 3])
def test_descriptor_against_the_fp32_oracle(dev, engine, group):
    """3 frames of 480 x 640 through CricaGPU.forward against the float64 head over the fp32
    oracle's final-normed tokens: two stages of 1e-9 whose amplitudes add, 4e-9."""
    f = R.e2e_fixture()
    ref = _oracle_descriptors(group)
    eng = copy.copy(engine)
    eng.group = group
    got = eng.forward(_dev(f["frames"], dev)).cpu().numpy()
    assert got.shape == (3, R.DIM) and got.dtype == np.float32
    err = [R.one_minus_cos(a, b) for a, b in zip(got, ref)]
    print(f"group {group}: 1 - cos {max(err):.3e} per frame {[f'{e:.2e}' for e in err]}")
    assert np.all(np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1) <= 1e-5)
    assert max(err) <= 4e-9


_oracle_tokens = {}


def _oracle_descriptors(group):
    """The fp32 oracle's tokens (computed once for both groupings), then the float64 head."""
    from oracle import vit as ovit
    f = R.e2e_fixture()
    sd = f["state_dict"]
    if "t" not in _oracle_tokens:
        osd = {k[len("backbone."):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items()
               if k.startswith("backbone.")}
        x = torch.cat([ovit.preprocess(fr) for fr in f["frames"]])
        _oracle_tokens["t"] = ovit.forward_tokens_with_cls(x, osd).numpy()
    return R.descriptor(_oracle_tokens["t"], sd, group)


# ------------------------------------------------------------ 6. the drop-in
def test_dropin_native_branch(dev, monkeypatch, frames7):
    """SemanticPlaceRecognition('cricavpr') with .vpr.native = True: 10752-dim unit float32
    descriptors from every entry point, the local-feature cache from the same forward, matches
    equal to the oracle retrieval loop over the returned descriptors, rerank unchanged."""
    from oracle import retrieval as oret
    monkeypatch.delenv("MLGATE_CRICAVPR_NATIVE", raising=False)
    monkeypatch.delenv("MLGATE_CRICAVPR_WEIGHTS", raising=False)
    imgs = list(frames7.cpu().numpy())
    t = [15.0 * i for i in range(6)]
    floors = [i % 2 for i in range(6)]
    spr = SemanticPlaceRecognition("cricavpr", device=str(dev), similarity_threshold=0.0)
    spr.vpr.native = True
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        spr.add_image(imgs[0], t[0], floors[0])
    assert any("synthetic" in str(w.message) and "CricaVPR" in str(w.message) for w in rec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spr.add_images(imgs[1:6], t[1:], floors[1:])
        X = spr.vpr.build_descriptor_matrix()
        one = spr.vpr.extract_descriptor(imgs[6])
        many = spr.vpr.extract_descriptors(imgs[5:7])
        qm = spr.vpr.query(imgs[6], timestamp=200.0, k=3, min_time_gap=50.0)
        got = spr.find_loop_closures(k=3)
        plain = CricaVPR(device=str(dev))
        plain.add_images(imgs[:6], t, floors)
    assert X.shape == (6, 10752) and X.dtype == np.float32 and spr.vpr._vit is None
    assert np.all(np.abs(np.linalg.norm(X.astype(np.float64), axis=1) - 1) <= 1e-5)
    assert one.shape == (10752,) and one.dtype == np.float32 and np.array_equal(many[1], one)
    assert np.array_equal(many[0], X[5])  # group 1: a frame's descriptor does not depend on the call
    ta, fl, hf = np.array(t), np.array(floors, np.int64), np.ones(6, np.uint8)
    rq, rm, rs, rv = oret.find_loop_closures(X, ta, fl, hf, spr.min_time_gap, 0.0, 3, True)
    assert len(got) == len(rq) > 0
    assert [m.query_idx for m in got] == rq.tolist() and [m.match_idx for m in got] == rm.tolist()
    assert [m.is_valid for m in got] == rv.astype(bool).tolist()
    assert np.max(np.abs(np.array([m.similarity for m in got]) - rs)) <= 4e-6
    ro, _ = oret.query(X, one, ta, 200.0, 3, 50.0)
    assert [m.match_idx for m in qm] == ro.tolist()
    # the rerank cache is the default branch's, bit for bit, so reranking is too
    assert plain.build_descriptor_matrix().shape == (6, 768) and sorted(spr.vpr._feature_cache) == list(range(6))
    for i in range(6):
        assert torch.equal(spr.vpr._feature_cache[i], plain._feature_cache[i])
    cands = [(j, 0.9 - 0.1 * j) for j in (1, 3, 4, 5)]
    assert spr.vpr.rerank_candidates(0, cands, top_k=3) == plain.rerank_candidates(0, cands, top_k=3)
    # a group of 3 through the drop-in: the engine's forward with group 3
    spr.vpr.cross_image_group = 3
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        grouped = spr.vpr.extract_descriptors(imgs[:6])
    eng = spr.vpr._crica
    assert eng.group == 3 and np.array_equal(grouped, eng.forward(frames7[:6]).cpu().numpy())
    assert not np.array_equal(grouped, X)


def test_environment_selects_the_branch(dev, monkeypatch, frames7):
    img = frames7[0].cpu().numpy()
    monkeypatch.setenv("MLGATE_CRICAVPR_NATIVE", "1")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert CricaVPR(device=str(dev)).extract_descriptor(img).shape == (10752,)
        forced = CricaVPR(device=str(dev))
        forced.native = False
        assert forced.extract_descriptor(img).shape == (768,) and forced._crica is None


# ------------------------------------------------------------ 7. malformed weight lists
def test_malformed_weight_lists_are_refused(dev, engine):
    """crica_forward and crica_encoder check every tensor of both lists before launching."""
    from weight_corruptions import assert_refused
    ops, vit = _native.ops(), engine._vit
    x = torch.zeros(1, 32, 32, 3, dtype=torch.uint8, device=dev)
    pooled = torch.zeros(1, 14, 768, device=dev)
    assert_refused(lambda b: ops.crica_forward(x, b, engine._head, 3.0, 322, vit.flags, 1, 1, False), vit._w, 0,
                   "patch_w")
    assert_refused(lambda b: ops.crica_forward(x, vit._w, b, 3.0, 322, vit.flags, 1, 1, False), engine._head, 8,
                   "layers[0].fc2_w")
    assert_refused(lambda b: ops.crica_encoder(pooled, b, 3.0, 1), engine._head, 12, "layers[1].in_w")
    head, p = pack_head(R.head_sd(), dev)
    assert p == 3.0 and all(torch.equal(a, b) for a, b in zip(head, engine._head))
    with pytest.raises(RuntimeError, match="expected 24 tensors, got 23"):
        ops.crica_encoder(pooled, head[:-1], 3.0, 1)
    with pytest.raises(RuntimeError):
        ops.crica_encoder(pooled, head, 0.0, 1)  # gem_p must be positive
    with pytest.raises(RuntimeError):
        ops.crica_encoder(pooled, head, 3.0, 33)
