"""End-to-end CricaVPR descriptor parity: HIP ViT-B/14 + GeM vs the float32 CPU oracle.

Tolerance (north star): descriptors within 1e-4 cosine of the oracle.  Weights are
seeded synthetic weights of the hub dinov2_vitb14 architecture (no network for the
real checkpoint: parity against the real weights is unpinned)."""
import numpy as np
import pytest
import torch

from mlgate.vit import VitB14
from mlgate.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu


def scene(rng, h=480, w=640):
    """Rectangles + noise, the synthetic-frame recipe of geometric_verification.py:755-774."""
    img = np.zeros((h, w, 3), np.uint8)
    for _ in range(30):
        x, y = rng.integers(0, w - 60), rng.integers(0, h - 60)
        ww, hh = rng.integers(20, 120), rng.integers(20, 120)
        img[y:y + hh, x:x + ww] = rng.integers(60, 255, 3)
    return np.clip(img.astype(np.int32) + rng.integers(0, 30, img.shape), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def sd():
    return synthetic_state_dict(0)


@pytest.fixture(scope="module")
def frames():
    rng = np.random.default_rng(1)
    return np.stack([scene(rng) for _ in range(3)] + [rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)])


def test_descriptor_cosine(dev, sd, frames):
    from oracle import vit as ovit
    torch.set_num_threads(8)
    eng = VitB14(sd, device="cuda", max_batch=4, precise=False)
    desc, local = eng.forward(torch.from_numpy(frames).to(dev), with_local=True)
    torch.cuda.synchronize()
    desc, local = desc.cpu(), local.cpu()
    osd = {k: torch.from_numpy(v) for k, v in sd.items()}
    for b in range(len(frames)):
        tok = ovit.forward_tokens(ovit.preprocess(frames[b]), osd)
        ref_d = ovit.gem(tok)[0]
        cos = torch.nn.functional.cosine_similarity(desc[b].double(), ref_d.double(), dim=0).item()
        assert 1 - cos < 1e-4, (b, cos)
        ref_l = tok[0, 1:]
        lc = torch.nn.functional.cosine_similarity(local[b].double(), ref_l.double(), dim=1)
        assert (1 - lc).max().item() < 1e-3
        assert local[b].shape == (528, 768)


def test_batch_split_consistent(dev, sd, frames):
    """Descriptors do not depend on how frames are batched (max_batch split)."""
    eng2 = VitB14(sd, device="cuda", max_batch=2, precise=False)
    eng4 = VitB14(sd, device="cuda", max_batch=4, precise=False)
    x = torch.from_numpy(frames).to(dev)
    d2, d4 = eng2.forward(x), eng4.forward(x)
    torch.cuda.synchronize()
    assert torch.allclose(d2, d4, rtol=0, atol=1e-6)


def test_gray_and_bgra_inputs(dev, sd, frames):
    from oracle import vit as ovit
    osd = {k: torch.from_numpy(v) for k, v in sd.items()}
    eng = VitB14(sd, device="cuda", max_batch=2, precise=False)
    gray = frames[:1, :, :, 1].copy()
    bgra = np.concatenate([frames[:1], np.full(frames[:1].shape[:3] + (1,), 255, np.uint8)], axis=-1)
    for f in (gray, bgra):
        d = eng.forward(torch.from_numpy(f).to(dev)).cpu()[0]
        ref = ovit.gem(ovit.forward_tokens(ovit.preprocess(f[0]), osd))[0]
        cos = torch.nn.functional.cosine_similarity(d.double(), ref.double(), dim=0).item()
        assert 1 - cos < 1e-4


def test_precise_split_descriptor_matches_fp32(dev, sd, frames):
    """MLG_VIT_SPLIT (VitB14(precise=True)): every GEMM / attention operand as a hi + lo
    bf16 pair, three MFMA products each.  Against the float32 oracle the descriptors agree
    to 1 - cos <= 1e-9 (the bf16 forward: ~1e-5) and the local features to 1e-7; the
    pairwise descriptor similarities to 1e-6 (the bf16 forward moves them by up to 3e-4,
    which is what reorders near-tied kNN neighbours at bench scale)."""
    from oracle import vit as ovit
    torch.set_num_threads(8)
    eng = VitB14(sd, device="cuda", max_batch=4, precise=True)
    desc, local = eng.forward(torch.from_numpy(frames).to(dev), with_local=True)
    torch.cuda.synchronize()
    desc, local = desc.cpu().double(), local.cpu().double()
    osd = {k: torch.from_numpy(v) for k, v in sd.items()}
    refs = []
    for b in range(len(frames)):
        tok = ovit.forward_tokens(ovit.preprocess(frames[b]), osd)
        refs.append(ovit.gem(tok)[0].double())
        cos = torch.nn.functional.cosine_similarity(desc[b], refs[-1], dim=0).item()
        assert 1 - cos < 1e-9, (b, 1 - cos)
        lc = torch.nn.functional.cosine_similarity(local[b], tok[0, 1:].double(), dim=1)
        assert (1 - lc).max().item() < 1e-7, (b, (1 - lc).max().item())
    R = torch.stack(refs)
    nrm = lambda X: X / X.norm(dim=1, keepdim=True)  # noqa: E731
    assert (nrm(desc) @ nrm(desc).T - nrm(R) @ nrm(R).T).abs().max().item() < 1e-6


def test_precise_batch_split_bit_identical(dev, sd, frames):
    """The split forward does not depend on how frames are batched, bit for bit."""
    x = torch.from_numpy(frames).to(dev)
    d2 = VitB14(sd, device="cuda", max_batch=2, precise=True).forward(x)
    d4 = VitB14(sd, device="cuda", max_batch=4, precise=True).forward(x)
    torch.cuda.synchronize()
    assert torch.equal(d2, d4)


def test_precise_batch_split_bit_identical_walking_tiles(dev, sd, frames):
    """The same with more output tiles than CUs, so that the persistent split GEMM
    (gemm_bf16.hip k_gemm256s) walks: a workgroup takes a second 256 x 256 tile and its
    last K-step prefetches that tile's operands.  16 frames in one batch are M = 8480
    token rows = 34 M-tiles (the last of 32 rows): qkv has 306 tiles and fc1 408."""
    x = torch.from_numpy(np.tile(frames, (4, 1, 1, 1))).to(dev)
    e16 = VitB14(sd, device="cuda", max_batch=16, precise=True)
    m_tiles = (len(x) * (e16.n_patches + 1) + 255) // 256
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert m_tiles * (3 * 768 // 256) > cus and m_tiles * (4 * 768 // 256) > cus
    d16 = e16.forward(x)
    d4 = VitB14(sd, device="cuda", max_batch=4, precise=True).forward(x)
    torch.cuda.synchronize()
    assert torch.equal(d16, d4)


def test_malformed_weight_list_is_refused(dev, sd):
    """vit_forward_into checks every tensor of its list before launching (weight_tables.h);
    `pos` is sized by image_size and the GEMM weights by the packing flag.  Every replacement
    is at least as large as what the flags ask for."""
    from mlgate import _native
    from mlgate.vit import pack_weights
    from weight_corruptions import assert_refused
    w = pack_weights(sd, dev, 23, False)
    x = torch.zeros(1, 32, 32, 3, dtype=torch.uint8, device=dev)
    desc = torch.empty(1, 768, device=dev)
    assert_refused(lambda b: _native.ops().vit_forward_into(x, b, 322, 0, 2, desc, None), w, 6, "blocks[0].qkv_w")
    with pytest.raises(RuntimeError, match=r"weights\[3\] \(pos\)"):
        _native.ops().vit_forward_into(x, w, 308, 0, 2, desc, None)  # 22 x 22 patches: a smaller table than pos
    # a list packed [W_hi | W_lo] for MLG_VIT_SPLIT, without the flag: every GEMM weight is twice the plain size
    # (the other way round, a plain list with the flag, is too short: tests/test_weight_lists_cpu.py)
    with pytest.raises(RuntimeError, match=r"weights\[0\] \(patch_w\)"):
        _native.ops().vit_forward_into(x, pack_weights(sd, dev, 23, True), 322, 0, 2, desc, None)
