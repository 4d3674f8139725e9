"""MixVPR's native branch on the GPU (csrc/mixvpr.hip, csrc/resnet.hip at side 320) against
the fp32 restatement (tests/mixvpr_restatement.py): bit-exact preprocessing, the fused
mixer head within 8x the bf16 operand-rounding floor of the fp32 head, the whole descriptor
within the trunk's bf16 bar, and the drop-in class."""
import warnings

import numpy as np
import pytest
import torch

import mixvpr_restatement as R
from mlgate import _native
from mlgate.mixvpr import MixVprGPU
from mlgate.resnet import ResNet50GPU
from mlgate.vpr import MixVPR, SemanticPlaceRecognition
from oracle import vit as ovit

pytestmark = pytest.mark.gpu

DESCRIPTOR_BAR = 4 * 1.09e-4  # 4x the 1 - cos measured on an MI355X (test_descriptor_matches_fp32_model)


@pytest.fixture(scope="module")
def engine(dev):
    return MixVprGPU(R.head_weights(), device=str(dev))


@pytest.mark.parametrize("shape", [(480, 640, 3), (540, 720, 3), (100, 90), (300, 200, 4), (320, 320, 3)])
def test_preprocess_bit_exact(dev, shape):
    rng = np.random.default_rng(shape[0] + len(shape))
    imgs = rng.integers(0, 256, (2,) + shape, dtype=np.uint8)
    t = torch.from_numpy(imgs).to(dev)
    got = _native.ops().mixvpr_preprocess(t if t.dim() == 4 else t.unsqueeze(-1)).cpu()
    assert got.shape == (2, 320, 320, 3) and got.dtype == torch.float32
    for b in range(2):
        want = ovit.preprocess(imgs[b], 320, swap_rb=True)[0].permute(1, 2, 0)
        assert torch.equal(got[b], want), (shape, b)


def _gpu_head(engine, dev, lo, hi):
    f = torch.from_numpy(R.head_features()[lo:hi]).to(dev).permute(0, 2, 1).contiguous()  # NHWC [B, 400, 1024]
    return engine.head(f).cpu().numpy()


@pytest.mark.parametrize("batch", [1, 3, 17])
def test_head_within_operand_rounding_of_fp32(engine, dev, batch):
    """B = 1: 16 row tiles, far fewer than CUs; B = 3: odd; B = 17: 272 tiles of 64 rows,
    more than the chip's 256 CUs.  Bar per image: 8 x e_emul, e_emul the 1 - cos between the
    CPU restatement with bf16-rounded GEMM operands and the fp32 restatement (about 8e-6)."""
    ref, e_emul = R.head_reference()
    got = _gpu_head(engine, dev, 0, batch)
    assert got.shape == (batch, 4096) and got.dtype == np.float32
    err = R.one_minus_cos(got, ref[:batch])
    print(f"B={batch}: 1 - cos to fp32 max {err.max():.3e}; e_emul {e_emul[:batch].min():.3e}..{e_emul[:batch].max():.3e}; "
          f"ratio max {np.max(err / e_emul[:batch]):.2f}")
    assert np.all(np.isfinite(got))
    assert np.all(err <= 8 * e_emul[:batch]), (err, e_emul[:batch])
    assert np.all(np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1) <= 1e-5)


def test_head_rows_are_independent_and_repeatable(engine, dev):
    three = _gpu_head(engine, dev, 0, 3)
    assert np.array_equal(three, _gpu_head(engine, dev, 0, 3))
    for b in range(3):
        assert np.array_equal(three[b], _gpu_head(engine, dev, b, b + 1)[0]), b
    assert np.array_equal(three, _gpu_head(engine, dev, 0, 17)[:3])


def test_descriptor_matches_fp32_model(engine, dev):
    """MixVprGPU.forward (preprocess, cropped trunk, head) on 3 seeded 480x640 frames against
    the full fp32 restatement.  The trunk's bf16 GEMMs dominate the error.  Measured on an
    MI355X: 1 - cos = 9.9e-5, 1.09e-4, 9.5e-5; the bar is 4x the maximum, well below the 2e-3 that
    tests/test_resnet_gpu.py holds for the same trunk's GAP descriptor."""
    sd = R.head_weights()
    rng = np.random.default_rng(1)
    imgs = rng.integers(0, 256, (3, 480, 640, 3), dtype=np.uint8)
    got = engine.forward(torch.from_numpy(imgs).to(dev)).cpu().numpy()
    ref = R.descriptor(sd, list(imgs)).numpy()
    err = R.one_minus_cos(got, ref)
    print("whole descriptor 1 - cos:", err)
    assert got.shape == (3, 4096)
    assert np.all(np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1) <= 1e-5)
    assert np.all(err <= DESCRIPTOR_BAR), err
    # batches beyond max_batch are chunked: same rows
    small = MixVprGPU(sd, device=str(dev), max_batch=2)
    assert np.array_equal(small.forward(torch.from_numpy(imgs).to(dev)).cpu().numpy(), got)


def test_dropin_native(dev, monkeypatch):
    monkeypatch.delenv("MLGATE_MIXVPR_NATIVE", raising=False)
    monkeypatch.delenv("MLGATE_MIXVPR_WEIGHTS", raising=False)
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    m = MixVPR(device=str(dev))
    m.native = True
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        d = m.extract_descriptor(img)
    msgs = [str(w.message) for w in rec]
    assert any("synthetic" in s for s in msgs), msgs
    assert not any("MixVPR not installed" in s for s in msgs), msgs
    assert d.shape == (4096,) and d.dtype == np.float32 and abs(np.linalg.norm(d.astype(np.float64)) - 1) <= 1e-5
    assert m.extract_descriptor(img[..., 0]).shape == (4096,)
    bgra = np.concatenate([img, np.full((480, 640, 1), 255, np.uint8)], axis=-1)
    assert np.array_equal(m.extract_descriptor(bgra), d)  # alpha is dropped
    assert np.array_equal(m.extract_descriptors([img, img[::-1].copy()])[0], d)

    # default (native unset, no environment variable): today's fallback
    f = MixVPR(device=str(dev))
    with pytest.warns(UserWarning):
        df = f.extract_descriptor(img)
    assert df.shape == (4096,) and np.all(df[2048:] == 0)
    gap = ResNet50GPU(device=str(dev)).forward_device(torch.from_numpy(img[None]).to(dev), 4096).cpu().numpy()[0]
    assert np.array_equal(df, gap)

    for kw in ({"descriptor_dim": 2048}, {"backbone": "efficientnet_b0"}):
        bad = MixVPR(device=str(dev), **kw)
        bad.native = True
        with pytest.raises(ValueError):
            bad.extract_descriptor(img)


def test_place_recognition_with_native_mixvpr(dev, monkeypatch):
    monkeypatch.setenv("MLGATE_MIXVPR_NATIVE", "1")
    rng = np.random.default_rng(3)
    frames = list(rng.integers(0, 256, (6, 240, 320, 3), dtype=np.uint8))
    frames[4] = frames[0].copy()
    spr = SemanticPlaceRecognition("mixvpr", device=str(dev))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spr.add_images(frames, [30.0 * i for i in range(6)], [1] * 6)
    assert spr.vpr._mix is not None and spr.vpr.descriptors[0].descriptor.shape == (4096,)
    of4 = [m for m in spr.find_loop_closures(k=5) if m.query_idx == 4]
    best = max(of4, key=lambda m: m.similarity)
    assert best.match_idx == 0 and best.similarity >= 0.9999, [(m.match_idx, m.similarity) for m in of4]


def test_malformed_weight_lists_are_refused(engine, dev):
    """mixvpr_forward and mixvpr_head check their lists before launching (weight_tables.h)."""
    from weight_corruptions import assert_refused
    ops = _native.ops()
    x = torch.zeros(1, 32, 32, 3, dtype=torch.uint8, device=dev)
    f = torch.zeros(1, 400, 1024, device=dev)
    assert_refused(lambda b: ops.mixvpr_forward(x, b, engine._head, 2), engine._trunk, 100, "blocks[12].w2")
    assert_refused(lambda b: ops.mixvpr_forward(x, engine._trunk, b, 2), engine._head, 0, "mix_w")
    assert_refused(lambda b: ops.mixvpr_head(f, b), engine._head, 0, "mix_w")
