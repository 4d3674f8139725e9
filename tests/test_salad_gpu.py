"""SALAD native branch on the GPU (mlgate.salad, csrc/salad.hip) vs the float32 oracle
(oracle/salad.py: serizba/salad's aggregator over the hub DINOv2 forward).

Tolerance: the backbone runs bf16 MFMA GEMMs / attention (1 - cos <= 1e-4 on the GeM
descriptor, tests/test_vit_gpu.py) and the aggregator's 1x1-conv MLPs bf16 operands with
f32 accumulation; the Sinkhorn, aggregation and normalisations run in f32.  Bar:
1 - cos <= 2e-3 on the 8448-dim descriptor, <= 2e-3 on its 256-dim token part and on
every 128-dim cluster block.  Parity against serizba/salad itself is unpinned (package
and checkpoint absent)."""
import numpy as np
import pytest
import torch

from mlgate.salad import SaladGPU
from mlgate.weights import salad_state_dict

pytestmark = pytest.mark.gpu


def scene(rng, h=480, w=640):
    img = np.zeros((h, w, 3), np.uint8)
    for _ in range(30):
        x, y = rng.integers(0, w - 60), rng.integers(0, h - 60)
        ww, hh = rng.integers(20, 120), rng.integers(20, 120)
        img[y:y + hh, x:x + ww] = rng.integers(60, 255, 3)
    return np.clip(img.astype(np.int32) + rng.integers(0, 30, img.shape), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def sd():
    return salad_state_dict(0)


@pytest.fixture(scope="module")
def frames():
    rng = np.random.default_rng(4)
    return np.stack([scene(rng) for _ in range(3)] + [rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)])


def _cos(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


def test_salad_descriptor_vs_oracle(dev, sd, frames):
    from oracle import salad as osalad
    torch.set_num_threads(8)
    eng = SaladGPU(sd, device="cuda", max_batch=4)
    got = eng.forward(torch.from_numpy(frames).to(dev))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == (4, 8448) and np.all(np.isfinite(got))
    osd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    for b in range(len(frames)):
        ref = osalad.extract_descriptor(frames[b], osd)
        assert abs(np.linalg.norm(got[b]) - 1) < 1e-5
        assert 1 - _cos(got[b], ref) <= 2e-3, (b, 1 - _cos(got[b], ref))
        assert 1 - _cos(got[b][:256], ref[:256]) <= 2e-3
        g_agg, r_agg = got[b][256:].reshape(128, 64), ref[256:].reshape(128, 64)
        worst = max(1 - _cos(g_agg[:, c], r_agg[:, c]) for c in range(64))
        assert worst <= 2e-3, (b, worst)


def test_salad_batch_split_consistent(dev, sd, frames):
    x = torch.from_numpy(frames).to(dev)
    d1 = SaladGPU(sd, device="cuda", max_batch=1).forward(x)
    d4 = SaladGPU(sd, device="cuda", max_batch=4).forward(x)
    torch.cuda.synchronize()
    assert torch.allclose(d1, d4, rtol=0, atol=1e-6)


def test_salad_dropin_native_and_fallback(dev, frames, monkeypatch):
    from mlgate.vpr import SALAD
    monkeypatch.setenv("MLGATE_SALAD_NATIVE", "1")
    s = SALAD(device=str(dev))
    with pytest.warns(UserWarning, match="SALAD weights"):
        d = s.extract_descriptor(frames[0])
    assert d.shape == (8448,) and d.dtype == np.float32 and abs(np.linalg.norm(d) - 1) < 1e-5
    batch = s.extract_descriptors(list(frames[:2]))
    assert np.allclose(batch[0], d, rtol=0, atol=1e-6)
    assert s.extract_descriptor(frames[1][..., 0]).shape == (8448,)  # gray -> GRAY2RGB
    with pytest.raises(ValueError):
        bad = SALAD(descriptor_dim=4096, device=str(dev))
        bad.native = True
        bad.extract_descriptor(frames[0])
    monkeypatch.delenv("MLGATE_SALAD_NATIVE")
    with pytest.warns(UserWarning, match="MixVPR fallback"):
        fb = SALAD(device=str(dev)).extract_descriptor(frames[0])
    assert fb.shape == (8448,) and np.all(fb[2048:] == 0)


def test_malformed_weight_lists_are_refused(dev, sd):
    """salad_forward checks both of its lists before launching (weight_tables.h)."""
    from mlgate import _native
    from mlgate.salad import IMAGE_SIZE, aggregator_list
    from mlgate.vit import pack_weights
    from weight_corruptions import assert_refused
    backbone = {k[len("backbone.model."):]: v for k, v in sd.items() if k.startswith("backbone.model.")}
    w = pack_weights(backbone, dev, IMAGE_SIZE // 14, False)
    agg, dust = aggregator_list(sd, dev)
    x = torch.zeros(1, 32, 32, 3, dtype=torch.uint8, device=dev)
    ops = _native.ops()
    assert_refused(lambda b: ops.salad_forward(x, w, b, dust, IMAGE_SIZE, 2), agg, 2, "w2")
    assert_refused(lambda b: ops.salad_forward(x, b, agg, dust, IMAGE_SIZE, 2), w, 167, "blocks[11].fc1_w")
