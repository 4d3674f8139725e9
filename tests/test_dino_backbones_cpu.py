"""The DINOv2 ViT-S / B / L-14 backbones on the CPU: the width-parametrised restatement against
the oracle and against transformers.Dinov2Model, the backbone table of mlgate.weights, the
mlg_dino_* entry points through ctypes without a device, the dino weight table, and the
drop-in's refusals."""
import ctypes
import re

import numpy as np
import pytest
import torch

import dino_restatement as R
from mlgate import _native, vit
from mlgate import weights as W
from mlgate.vpr import AnyLoc, CricaVPR
from oracle import vit as ovit

S14, B14, L14 = "dinov2_vits14", "dinov2_vitb14", "dinov2_vitl14"
CPU = torch.device("cpu")


# ------------------------------------------------------------------ the restatement
def test_restatement_equals_the_oracle_at_vitb():
    sd = W.synthetic_state_dict(3)
    x = ovit.preprocess(np.random.default_rng(0).integers(0, 256, (480, 640, 3), dtype=np.uint8), 322)
    ours = R.forward_tokens(x, sd, B14)
    ref = ovit.forward_tokens(x, sd)
    assert ours.shape == (1, 529, 768) and torch.equal(ours, ref)
    assert torch.equal(R.gem(ours), ovit.gem(ref))


def hf_model(sd, backbone):
    from transformers import Dinov2Config, Dinov2Model
    E, depth, heads, mlp = W.backbone_config(backbone)
    cfg = Dinov2Config(hidden_size=E, num_hidden_layers=depth, num_attention_heads=heads, mlp_ratio=4,
                       intermediate_size=mlp, patch_size=14, image_size=518, layer_norm_eps=1e-6, hidden_act="gelu",
                       qkv_bias=True, layerscale_value=1.0)
    m = Dinov2Model(cfg).eval()
    t = {k: torch.from_numpy(v) for k, v in sd.items()}
    hf = {
        "embeddings.cls_token": t["cls_token"],
        "embeddings.position_embeddings": t["pos_embed"],
        "embeddings.patch_embeddings.projection.weight": t["patch_embed.proj.weight"],
        "embeddings.patch_embeddings.projection.bias": t["patch_embed.proj.bias"],
        "embeddings.mask_token": torch.zeros(1, E),
        "layernorm.weight": t["norm.weight"],
        "layernorm.bias": t["norm.bias"],
    }
    for i in range(depth):
        p, q = f"blocks.{i}.", f"encoder.layer.{i}."
        w, b = t[p + "attn.qkv.weight"], t[p + "attn.qkv.bias"]
        for j, nm in enumerate(("query", "key", "value")):
            hf[q + f"attention.attention.{nm}.weight"] = w[j * E:(j + 1) * E]
            hf[q + f"attention.attention.{nm}.bias"] = b[j * E:(j + 1) * E]
        hf[q + "attention.output.dense.weight"] = t[p + "attn.proj.weight"]
        hf[q + "attention.output.dense.bias"] = t[p + "attn.proj.bias"]
        hf[q + "layer_scale1.lambda1"] = t[p + "ls1.gamma"]
        hf[q + "layer_scale2.lambda1"] = t[p + "ls2.gamma"]
        for nm in ("norm1", "norm2"):
            hf[q + f"{nm}.weight"] = t[p + f"{nm}.weight"]
            hf[q + f"{nm}.bias"] = t[p + f"{nm}.bias"]
        for nm in ("fc1", "fc2"):
            hf[q + f"mlp.{nm}.weight"] = t[p + f"mlp.{nm}.weight"]
            hf[q + f"mlp.{nm}.bias"] = t[p + f"mlp.{nm}.bias"]
    missing, unexpected = m.load_state_dict(hf, strict=False)
    assert not unexpected and not [k for k in missing if "mask_token" not in k], (missing, unexpected)
    return m


@pytest.mark.slow
@pytest.mark.parametrize("backbone", [S14, L14])
def test_restatement_matches_transformers_dinov2(backbone):
    """The bar of tests/test_oracle_vit.py: atol 2e-4 on tokens of magnitude ~5, at 518 where the
    position-embedding resampling is the identity."""
    torch.set_num_threads(8)
    sd = W.synthetic_state_dict(3, backbone)
    m = hf_model(sd, backbone)
    x = ovit.preprocess(np.random.default_rng(0).integers(0, 256, (480, 640, 3), dtype=np.uint8), 518)
    with torch.no_grad():
        ref = m(pixel_values=x).last_hidden_state[:, 1:]
    ours = R.forward_tokens(x, sd, backbone)
    assert ours.shape == ref.shape == (1, 1369, W.backbone_config(backbone)[0])
    print(f"{backbone}: max |restatement - transformers| = {(ours - ref).abs().max():.3e}")
    assert torch.allclose(ours, ref, rtol=0, atol=2e-4), (ours - ref).abs().max()


# ------------------------------------------------------------------------- weights
def test_vitb_synthetic_weights_are_unchanged_by_the_backbone_argument():
    a, b = W.synthetic_state_dict(5), W.synthetic_state_dict(5, B14)
    assert list(a) == list(b)
    assert all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in a)
    assert W.hub_keys() == W.hub_keys(B14) and len(W.hub_keys()) == 6 + 12 * 14
    assert W.BACKBONES[B14] == (W.EMBED, W.DEPTH, W.HEADS, W.MLP) == (768, 12, 12, 3072)


@pytest.mark.parametrize("backbone,E,depth,heads", [(S14, 384, 12, 6), (L14, 1024, 24, 16)])
def test_key_lists_and_shapes(backbone, E, depth, heads):
    assert W.backbone_config(backbone) == (E, depth, heads, 4 * E) and heads * 64 == E
    sd = W.synthetic_state_dict(1, backbone)
    keys = W.hub_keys(backbone)
    assert sorted(sd) == sorted(keys) and len(keys) == 6 + depth * 14
    assert f"blocks.{depth - 1}.ls2.gamma" in sd and f"blocks.{depth}.norm1.weight" not in sd
    assert {k: v.shape for k, v in sd.items()} == W.hub_shapes(backbone)
    assert all(v.dtype == np.float32 for v in sd.values())
    assert sd["cls_token"].shape == (1, 1, E) and sd["pos_embed"].shape == (1, 1370, E)
    assert sd["patch_embed.proj.weight"].shape == (E, 3, 14, 14)
    assert sd["blocks.0.attn.qkv.weight"].shape == (3 * E, E) and sd["blocks.0.mlp.fc2.weight"].shape == (E, 4 * E)


def test_unknown_backbones_are_refused_listing_the_three():
    for name in ("dinov2_vitg14", "dinov2_vitb14_reg", "resnet50"):
        for call in (W.backbone_config, W.hub_keys, lambda n: W.synthetic_state_dict(0, n),
                     lambda n: W.resolve_state_dict(None, 0, n)):
            with pytest.raises(ValueError) as e:
                call(name)
            assert name in str(e.value) and all(n in str(e.value) for n in (S14, B14, L14))


def test_checkpoint_of_another_width_is_refused(tmp_path, monkeypatch):
    path = tmp_path / "vitb.pth"
    torch.save({k: torch.from_numpy(v) for k, v in W.synthetic_state_dict(0).items()}, path)
    monkeypatch.delenv("MLGATE_DINOV2_WEIGHTS", raising=False)
    sd, source = W.resolve_state_dict(str(path))  # as ViT-B it loads
    assert source == str(path) and np.array_equal(sd["norm.bias"], W.synthetic_state_dict(0)["norm.bias"])
    for backbone, shape in ((S14, "(1, 1, 384)"), (L14, "(1, 1, 1024)")):
        for call in (lambda: W.load_hub_state_dict(str(path), backbone),
                     lambda: W.resolve_state_dict(str(path), backbone=backbone)):
            with pytest.raises(ValueError) as e:
                call()
            msg = str(e.value)
            assert backbone in msg and "cls_token" in msg and "(1, 1, 768)" in msg and shape in msg
    monkeypatch.setenv("MLGATE_DINOV2_WEIGHTS", str(path))
    with pytest.raises(ValueError, match=r"dinov2_vits14.*cls_token"):
        W.resolve_state_dict(backbone=S14)
    # same width, fewer blocks: the missing keys are named
    short = {k: v for k, v in W.synthetic_state_dict(0, L14).items() if not k.startswith("blocks.23.")}
    with pytest.raises(KeyError, match=r"dinov2_vitl14.*blocks\.23\."):
        W.check_state_dict(short, L14)


# ----------------------------------------------------------- the C ABI, without a device
EINVAL, ENOMEM = -1, -3
P, I = ctypes.c_void_p, ctypes.c_int


class DinoWeights(ctypes.Structure):  # include/mlgate.h mlg_dino_weights
    _fields_ = [("struct_size", ctypes.c_uint32), ("abi_version", ctypes.c_uint32), ("embed", I), ("depth", I),
                ("heads", I), ("patch_w", P), ("patch_b", P), ("cls", P), ("pos", P), ("blocks", P), ("norm_w", P),
                ("norm_b", P), ("packing", I)]


class Abi:
    """Dummy non-null pointers (never dereferenced: every refusal below comes before the first
    HIP call) and a well-formed mlg_dino_weights."""

    def __init__(self):
        self.L = _native.lib()
        self._buf = ctypes.create_string_buffer(1 << 16)
        self.d = P((ctypes.addressof(self._buf) + 255) & ~255)
        self.blocks = (P * (24 * 14))(*([self.d.value] * (24 * 14)))

    def weights(self, embed=384, depth=12, heads=6, packing=4, **over):
        w = DinoWeights()
        w.struct_size, w.abi_version = ctypes.sizeof(DinoWeights), 3
        w.embed, w.depth, w.heads, w.packing = embed, depth, heads, packing
        for f in ("patch_w", "patch_b", "cls", "pos", "norm_w", "norm_b"):
            setattr(w, f, self.d.value)
        w.blocks = ctypes.cast(self.blocks, P).value
        for k, v in over.items():
            setattr(w, k, v)
        return w

    def forward(self, w, flags=4, frames=True, ws=True, desc=True, ws_bytes=None, batch=2, size=322):
        need = self.L.mlg_dino_workspace_bytes(w.embed, batch, size)
        return self.L.mlg_dino_forward(ctypes.byref(w), self.d if frames else None, batch, 480, 640, 3, 480 * 640 * 3,
                                       size, flags, self.d if ws else None, need if ws_bytes is None else ws_bytes,
                                       self.d if desc else None, None, None)


def carved_bytes(embed, batch, size):
    """include/mlgate.h's layout of the workspace, restated: every buffer rounded up to 256 bytes."""
    T = 1 + (size // 14) ** 2
    rows, tpad = batch * T, (T + 63) // 64 * 64
    qkv = 2 * (embed // 64) * batch * tpad * 64 * 2
    bufs = [batch * (T - 1) * 768 * 2 * 2, rows * embed * 4, rows * embed * 2 * 2, qkv, qkv, qkv,
            rows * embed * 2 * 2, rows * 4 * embed * 2 * 2, batch * 8 * embed * 4, batch * 5 * 4]
    return sum((b + 255) // 256 * 256 for b in bufs)


def test_workspace_query():
    L = _native.lib()
    for embed in (384, 768, 1024):
        for B, S in ((1, 322), (3, 322), (64, 322), (1, 518), (7, 224), (246, 322), (1, 14)):
            assert L.mlg_dino_workspace_bytes(embed, B, S) == carved_bytes(embed, B, S), (embed, B, S)
    for B, S in ((1, 322), (3, 322), (64, 322), (1, 518), (7, 224)):
        assert L.mlg_dino_workspace_bytes(768, B, S) == L.mlg_vit_workspace_bytes(B, S) > 0
        assert 0 < L.mlg_dino_workspace_bytes(384, B, S) < L.mlg_vit_workspace_bytes(B, S)
        assert L.mlg_dino_workspace_bytes(1024, B, S) > L.mlg_vit_workspace_bytes(B, S)
    for embed in (512, 0, -384, 1536, 385):
        assert L.mlg_dino_workspace_bytes(embed, 2, 322) == 0
    assert L.mlg_dino_workspace_bytes(384, 0, 322) == 0 and L.mlg_dino_workspace_bytes(384, 2, 320) == 0


def test_forward_refusals_come_before_any_gpu_call():
    a = Abi()
    ok = a.weights()
    assert a.forward(ok, ws_bytes=a.L.mlg_dino_workspace_bytes(384, 2, 322) - 1) == ENOMEM  # a whole struct gets this far
    # a foreign struct head
    assert a.forward(a.weights(struct_size=ctypes.sizeof(DinoWeights) - 8)) == EINVAL
    assert a.forward(a.weights(abi_version=2)) == EINVAL
    # not a row of the table
    for cfg in (dict(embed=512, heads=8), dict(embed=384, heads=12), dict(embed=384, depth=24),
                dict(embed=1024, depth=12, heads=16), dict(embed=768, depth=12, heads=6), dict(blocks=None),
                dict(embed=0, heads=0), dict(depth=0)):
        assert a.forward(a.weights(**cfg)) == EINVAL, cfg
    # packing against the flag
    assert a.forward(a.weights(packing=0), flags=4) == EINVAL
    assert a.forward(a.weights(packing=4), flags=0) == EINVAL
    # null pointers, bad sizes
    assert a.forward(ok, frames=False) == EINVAL
    assert a.forward(ok, ws=False) == EINVAL
    assert a.forward(ok, desc=False) == EINVAL
    assert a.L.mlg_dino_forward(None, a.d, 2, 480, 640, 3, 480 * 640 * 3, 322, 4, a.d, 1 << 40, a.d, None, None) == EINVAL
    assert a.forward(ok, batch=0, ws_bytes=1 << 40) == EINVAL and a.forward(ok, size=320, ws_bytes=1 << 40) == EINVAL
    for cfg in (dict(embed=768, depth=12, heads=12), dict(embed=1024, depth=24, heads=16)):
        w = a.weights(**cfg)
        assert a.forward(w, ws_bytes=a.L.mlg_dino_workspace_bytes(w.embed, 2, 322) - 1) == ENOMEM


# ----------------------------------------------------------------- the weight table
EMBED = {S14: 384, B14: 768, L14: 1024}
_lists = {}


def packed(backbone, precise):
    if (backbone, precise) not in _lists:
        _lists[backbone, precise] = vit.pack_weights(W.synthetic_state_dict(0, backbone), CPU, 23, precise, backbone)
    return list(_lists[backbone, precise])


def check(w, backbone, split):
    _native.ops().dino_weights_check(w, EMBED[backbone], split)


@pytest.mark.parametrize("backbone", [S14, B14, L14])
@pytest.mark.parametrize("precise", [False, True])
def test_packed_list_is_accepted(backbone, precise):
    w = packed(backbone, precise)
    assert len(w) == 6 + 14 * W.backbone_config(backbone)[1]
    check(w, backbone, precise)
    if backbone == B14:  # the list VitB14 packs, by the table vit_forward_into checks
        _native.ops().weights_check("vit_split" if precise else "vit", w)


def test_vits_split_packing_pads_the_tail_rows_with_zeros():
    """1152, 384 rows -> 1280, 512 (the split GEMM's 256-column tile); plain lists have no padding."""
    w, plain = packed(S14, True), packed(S14, False)
    shapes = {0: (512, 1536), 6: (1280, 768), 8: (512, 768), 13: (1536, 768), 15: (512, 3072)}
    for i, shp in shapes.items():
        assert tuple(w[i].shape) == shp, (i, w[i].shape)
    for i, rows in ((0, 384), (6, 1152), (8, 384), (15, 384)):
        assert plain[i].shape[0] == rows and not w[i][rows:].float().abs().any() and w[i][:rows].float().abs().any()
        assert torch.equal(w[i][:rows, :plain[i].shape[1]], plain[i])  # the hi half is the plain bf16 weight


def test_wrong_width_or_depth_is_refused_naming_the_first_wrong_tensor():
    with pytest.raises(RuntimeError, match=re.escape("dino weights[0] (patch_w)") + ".*got 1179648 elements"):
        check(packed(B14, True), S14, True)  # a ViT-B list as ViT-S
    with pytest.raises(RuntimeError, match=re.escape("dino weights[0] (patch_w)") + ".*got 294912 elements"):
        check(packed(S14, False), B14, False)
    w = packed(L14, True)
    n = len(w)
    with pytest.raises(RuntimeError, match=f"expected {n} tensors, got {n - 14}"):
        check(w[:4 + 23 * 14] + w[-2:], L14, True)  # one block short
    with pytest.raises(RuntimeError, match=re.escape("weights[0] (patch_w)") + ".*with 786432 elements.*got 294912"):
        check(packed(S14, False), S14, True)  # plain packing against the split table: 2 x 512 x 768
    w = packed(S14, True)
    w[8] = w[8][:384].contiguous()  # proj_w without its padding rows
    with pytest.raises(RuntimeError, match=re.escape("weights[8] (blocks[0].proj_w)") + ".*with 393216 elements.*got 294912"):
        check(w, S14, True)
    w = packed(L14, False)
    w[4 + 23 * 14 + 9] = w[4 + 23 * 14 + 9].float()
    with pytest.raises(RuntimeError, match=re.escape("(blocks[23].fc1_w)") + ".*bf16.*got f32"):
        check(w, L14, False)
    with pytest.raises(RuntimeError, match="embed must be 384"):
        _native.ops().dino_weights_check(packed(S14, False), 512, False)


# ---------------------------------------------------------------------- the drop-in
def test_dropin_refuses_unsupported_backbones_on_first_use():
    img = np.zeros((32, 32, 3), np.uint8)
    for m, name in ((CricaVPR(backbone="dinov2_vitg14"), "dinov2_vitg14"),
                    (AnyLoc(backbone="dinov2_vitb14_reg"), "dinov2_vitb14_reg")):
        for call in (lambda: m.extract_descriptor(img), lambda: m.extract_descriptors([img])):
            with pytest.raises(ValueError) as e:
                call()
            assert name in str(e.value) and all(n in str(e.value) for n in (S14, B14, L14)), str(e.value)


@pytest.mark.parametrize("backbone", [S14, L14])
def test_native_branches_still_refuse_other_widths(backbone, monkeypatch):
    for var in ("MLGATE_CRICAVPR_NATIVE", "MLGATE_ANYLOC_NATIVE"):
        monkeypatch.delenv(var, raising=False)
    img = np.zeros((32, 32, 3), np.uint8)
    c = CricaVPR(backbone=backbone)
    c.native = True
    a = AnyLoc(backbone=backbone)
    a.native = True
    for m in (c, a):
        with pytest.raises(ValueError, match=backbone + ".*dinov2_vitb14"):
            m.extract_descriptor(img)
