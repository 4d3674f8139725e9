"""MixVPR's native branch, host side (no GPU): the checkpoint resolver, the projection fold
the kernels rely on, the sensitivity of the synthetic weights (so the GPU bars of
tests/test_mixvpr_gpu.py can bite), and the C ABI's argument checks."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import mixvpr_restatement as R
from mlgate import _native, weights
from mlgate.mixvpr import NPAD, pack_head


@pytest.fixture(scope="module")
def sd():
    return R.head_weights()


def test_synthetic_state_dict_has_the_checkpoint_keys(sd):
    keys = weights.mixvpr_keys()
    assert list(sd) == keys and len(set(keys)) == len(keys)
    assert not any("layer4" in k or ".fc." in k for k in keys)
    for k, shp in weights.mixvpr_aggregator_shapes().items():
        assert sd["aggregator." + k].shape == shp and sd["aggregator." + k].dtype == np.float32, k
    assert sd["backbone.model.conv1.weight"].shape == (64, 3, 7, 7)
    assert sd["backbone.model.layer3.5.conv3.weight"].shape == (1024, 256, 1, 1)
    rn = weights.resnet50_state_dict(0)  # the trunk is the fallback generator's layers 1-3
    assert np.array_equal(sd["backbone.model.layer3.0.downsample.0.weight"], rn["layer3.0.downsample.0.weight"])
    # every aggregator tensor is drawn to matter: no zero biases, no identity LayerNorm
    for k in weights.mixvpr_aggregator_shapes():
        v = sd["aggregator." + k]
        assert np.std(v) > 0.01, k


def test_checkpoint_loader(sd, tmp_path):
    t = {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    extra = dict(t)
    extra["backbone.model.layer4.0.conv1.weight"] = torch.zeros(512, 1024, 1, 1)
    extra["backbone.model.fc.weight"] = torch.zeros(10, 2048)
    torch.save({"state_dict": extra, "epoch": 3}, tmp_path / "wrapped.ckpt")
    torch.save(t, tmp_path / "bare.pth")
    for name in ("wrapped.ckpt", "bare.pth"):
        got = weights.load_mixvpr_state_dict(str(tmp_path / name))
        assert list(got) == weights.mixvpr_keys()
        assert all(np.array_equal(got[k], sd[k]) for k in got)
    got, src = weights.resolve_mixvpr_state_dict(str(tmp_path / "bare.pth"))
    assert src.endswith("bare.pth") and np.array_equal(got["aggregator.row_proj.bias"], sd["aggregator.row_proj.bias"])
    broken = dict(t)
    del broken["aggregator.mix.2.mix.3.weight"]
    torch.save(broken, tmp_path / "broken.pth")
    with pytest.raises(KeyError):
        weights.load_mixvpr_state_dict(str(tmp_path / "broken.pth"))


def test_resolver_falls_back_to_seeded_synthetic(monkeypatch):
    monkeypatch.delenv("MLGATE_MIXVPR_WEIGHTS", raising=False)
    a, src = weights.resolve_mixvpr_state_dict(None, seed=3)
    assert src == "synthetic(seed=3)"
    assert np.array_equal(a["aggregator.channel_proj.bias"], weights.mixvpr_state_dict(3)["aggregator.channel_proj.bias"])


def _packed_head_f64(pack, x):
    """The head as the kernels evaluate it, from the packed arrays, in numpy float64:
    mixer blocks on the unpacked [416][416] matrices, row_proj first, then channel_proj with
    the bc * s term.  x [B, 1024, 400] -> [B, 4096]."""
    mix_w, mix_p, row_w, chan_w, chan_b, row_s, row_b = [np.asarray(a, np.float64) for a in pack]
    x = np.concatenate([np.asarray(x, np.float64), np.zeros(x.shape[:2] + (NPAD - R.HW,))], axis=-1)
    valid = np.arange(NPAD) < R.HW
    for i in range(R.DEPTH):
        w1, w2 = (mix_w[i, j].transpose(1, 0, 2).reshape(NPAD, NPAD) for j in range(2))  # undo pack_kstep
        g, b, b1, b2 = (mix_p[i, j, :NPAD] for j in range(4))
        mean = x[..., :R.HW].mean(-1, keepdims=True)
        var = ((x[..., :R.HW] - mean) ** 2).mean(-1, keepdims=True)
        t = np.where(valid, (x - mean) / np.sqrt(var + 1e-5) * g + b, 0.0)
        x = x + np.maximum(t @ w1.T + b1, 0.0) @ w2.T + b2
    assert np.all(x[..., R.HW:] == 0)  # the padding stays zero through every block
    P = x @ row_w[:, :NPAD].T  # [B, 1024, 4]
    out = np.einsum("oc,bcr->bor", chan_w, P) + chan_b[None, :, None] * row_s[None, None, :] + row_b
    out = out.reshape(len(x), -1)
    return out / np.linalg.norm(out, axis=-1, keepdims=True)


def test_projection_fold_equals_reference_order(sd):
    """row_proj before channel_proj (with bc[o] * s[r]) = the reference's order, to the fp32
    restatement's own rounding."""
    rng = np.random.default_rng(9)
    x = np.maximum(rng.standard_normal((2, R.C, R.HW)), 0).astype(np.float32)
    ref = R.head(sd, x).numpy()
    got = _packed_head_f64(pack_head(sd), x)
    d = R.one_minus_cos(got, ref)
    print("fold 1 - cos:", d)
    assert np.all(d <= 1e-7), d
    ref64 = R.head(sd, x, dtype=torch.float64).numpy()
    assert np.all(R.one_minus_cos(got, ref64) <= 1e-12)


def test_every_term_moves_the_descriptor(sd):
    """Dropping any one mixer block, or b1 / b2 / the LayerNorm affine / channel_proj.bias /
    row_proj.bias, moves the fp32 descriptor by at least 10x the GPU head bar (8 x e_emul) on
    the head test's own inputs -- a kernel that forgot the term could not pass that bar."""
    n = 2
    ref, e_emul = R.head_reference(n)
    f = R.head_features()[:n]
    assert np.all(e_emul > 1e-7) and np.all(e_emul < 1e-4), e_emul  # the bf16 operand floor, about 8e-6
    for term in R.OMITTABLE:
        d = R.one_minus_cos(R.head(sd, f, omit=term).numpy(), ref)
        print(term, d, "bar x10:", 80 * e_emul)
        assert np.all(d >= 10 * 8 * e_emul), (term, d, e_emul)


def test_abi_workspace_and_struct_head():
    L = _native.lib()
    assert L.mlg_mixvpr_workspace_bytes(2, 480, 640) > 0
    assert L.mlg_mixvpr_workspace_bytes(0, 480, 640) == 0
    assert L.mlg_mixvpr_workspace_bytes(-1, 480, 640) == 0
    assert L.mlg_mixvpr_workspace_bytes(2, 0, 640) == 0
    # a batch twice as large needs about twice the workspace
    assert L.mlg_mixvpr_workspace_bytes(4, 480, 640) > 1.9 * L.mlg_mixvpr_workspace_bytes(2, 480, 640)
    dummy = ctypes.create_string_buffer(4096)
    d = ctypes.cast(dummy, ctypes.c_void_p)
    heads = {"truncated": struct.pack("<II", 16, 3), "other_version": struct.pack("<II", 8 * 1024, 2),
             "v2_pointer_first": struct.pack("<Q", 0x7F1234567890), "zeros": bytes(8)}
    for name, head in heads.items():
        buf = ctypes.create_string_buffer(head + bytes(64 * 1024))  # room: never read past the head
        w = ctypes.cast(buf, ctypes.c_void_p)
        assert L.mlg_mixvpr_forward(w, d, 1, 480, 640, 3, 921600, d, 1 << 30, d, None) == -1, name
        assert L.mlg_op_mixvpr_head(w, d, 1, d, None) == -1, name
    # a well-formed head with null tables, and invalid sizes, are refused before any device work
    ok = ctypes.create_string_buffer(64 * 1024)
    size = 8 + 2 * 8 + 13 * 8 * 8 + 7 * 8
    ok[:8] = struct.pack("<II", size, 3)
    w = ctypes.cast(ok, ctypes.c_void_p)
    assert L.mlg_mixvpr_forward(w, d, 1, 480, 640, 3, 921600, d, 1 << 30, d, None) == -1
    assert L.mlg_op_mixvpr_head(w, d, 1, d, None) == -1
    assert L.mlg_op_mixvpr_preprocess(d, 0, 480, 640, 3, 921600, d, None) == -1
    assert L.mlg_op_mixvpr_preprocess(d, 1, 480, 640, 2, 921600, d, None) == -1
    assert L.mlg_op_mixvpr_preprocess(d, 1, 480, 640, 3, 100, d, None) == -1


def test_native_refuses_other_configurations_without_a_device():
    from mlgate.vpr import MixVPR
    img = np.zeros((48, 64, 3), np.uint8)
    for kw in ({"descriptor_dim": 2048}, {"backbone": "efficientnet_b0"}):
        m = MixVPR(device="cuda", **kw)
        m.native = True
        with pytest.raises(ValueError):
            m.extract_descriptor(img)
    assert MixVPR().native is None
