"""CricaVPR's native branch without a GPU: the float64 restatement (tests/crica_restatement.py)
against torch.nn.TransformerEncoder, the region slices, the conditions the GPU tests'
fixtures must meet (asserted here so tests/test_crica_gpu.py can rely on them), the weight
packer against the C++ table, the checkpoint loader, the C ABI's argument checks (all before
any GPU call, so they run here with dummy pointers) and the drop-in's argument errors."""
import ctypes
import re
import sys

import numpy as np
import pytest
import torch

import crica_restatement as R
from mlgate import _native
from mlgate import weights as W
from mlgate.vpr import CricaVPR

CPU = torch.device("cpu")


# ------------------------------------------------------------------ the restatement
def _torch_encoder(sd):
    layer = torch.nn.TransformerEncoderLayer(d_model=768, nhead=16, dim_feedforward=2048, activation="gelu",
                                             dropout=0.1, batch_first=False)
    enc = torch.nn.TransformerEncoder(layer, num_layers=2, enable_nested_tensor=False).double().eval()
    enc.load_state_dict({k[len("encoder."):]: torch.from_numpy(np.asarray(v)).double() for k, v in sd.items()
                         if k.startswith("encoder.")})
    return enc


@pytest.mark.parametrize("B, group", [(2, 1), (7, 3), (32, 32)])
def test_restatement_equals_torch_transformer_encoder(B, group):
    """nn.TransformerEncoder applied to [n, 14, 768] with batch_first=False, group by group."""
    sd, x = R.head_sd(), R.pooled_fixture(B)
    enc = _torch_encoder(sd)
    got = R.encode(x, sd, group)
    with torch.no_grad():
        for f0, f1 in R.groups(B, group):
            y = enc(torch.tensor(x[f0:f1], dtype=torch.float64)).numpy().reshape(f1 - f0, R.DIM)
            y /= np.maximum(np.linalg.norm(y, axis=1, keepdims=True), 1e-12)
            assert np.max(np.abs(got[f0:f1] - y)) <= 1e-12
    assert np.allclose(np.linalg.norm(got, axis=1), 1, atol=1e-12)


def test_group_of_one_is_out_proj_of_v():
    """A single image: softmax over one key is 1, so the attention block is LN(x + out_proj(V))."""
    sd, x = R.head_sd(), R.pooled_fixture(1)[0].astype(np.float64)
    k = lambda s: np.asarray(sd["encoder.layers.0." + s], np.float64)  # noqa: E731
    v = x @ k("self_attn.in_proj_weight")[2 * 768:].T + k("self_attn.in_proj_bias")[2 * 768:]
    x1 = R.layernorm(x + v @ k("self_attn.out_proj.weight").T + k("self_attn.out_proj.bias"), k("norm1.weight"),
                     k("norm1.bias"), 1e-5)
    h = x1 @ k("linear1.weight").T + k("linear1.bias")
    h = h * 0.5 * (1 + torch.erf(torch.from_numpy(h / np.sqrt(2.0))).numpy())
    want = R.layernorm(x1 + h @ k("linear2.weight").T + k("linear2.bias"), k("norm2.weight"), k("norm2.bias"), 1e-5)
    assert np.max(np.abs(R._layer(x[None], sd, 0, "f64")[0] - want)) <= 1e-12


@pytest.mark.parametrize("g", [12, 16, 23])
def test_regions_tile_each_level_once(g):
    regs = R.regions(g)
    assert len(regs) == 13
    for level in (regs[:4], regs[4:]):
        cover = np.zeros((g, g), int)
        for rs, cs in level:
            cover[rs, cs] += 1
            assert cover[rs, cs].size > 0
        assert np.all(cover == 1)
    if g == 23:  # upstream's literal slices on the reference's 322 input: uneven bands
        assert [(r.stop - r.start, c.stop - c.start) for r, c in regs[:4]] == [(8, 8), (8, 15), (15, 8), (15, 15)]
        assert [c.stop - c.start for _, c in regs[4:7]] == [5, 6, 12]


def test_pyramid_rows():
    """Row 0 is the normed CLS token; every patch, patch 0 included, reaches the pyramid."""
    x, nw, nb = R.pool_fixture(1, 16)
    normed = R.layernorm(x, nw, nb, 1e-6)
    rows = R.pool(x, nw, nb, 3.0)
    assert rows.shape == (1, 14, 768) and np.array_equal(rows[0, 0], normed[0, 0])
    moved = np.array(x)
    moved[0, 1] += 1.0  # patch token 0 sits in region 1 and in region 5 only
    changed = np.any(R.pool(moved, nw, nb, 3.0) != rows, axis=-1)[0]
    assert changed.tolist() == [r in (1, 5) for r in range(14)]


# ------------------------------------------------------------------ what the GPU tests rely on
def test_pool_fixture_has_negative_channels_and_a_zero_token():
    for B, g, _ in R.POOL_CASES:
        x, nw, nb = R.pool_fixture(B, g)
        normed = R.layernorm(x, nw, nb, 1e-6)
        assert np.mean(normed[:, 1:] < 0) > 0.3  # the clamp at 1e-6 is at work
        assert not np.any(x[0, 4]) and np.all(np.isfinite(R.pool(x, nw, nb, 2.5)))
        assert x.dtype == np.float32 and x.shape == (B, 1 + g * g, 768)


def test_a_wrong_grouping_cannot_pass():
    """With the synthetic head a frame's float64 descriptor in a group of 4 differs from the
    same frame alone by 1 - cos >= 1e-3: a million times the GPU tests' bar."""
    x, sd = R.pooled_fixture(7), R.head_sd()
    alone, four, three = R.encode(x, sd, 1), R.encode(x, sd, 4), R.encode(x, sd, 3)
    for b in range(7):
        assert R.one_minus_cos(alone[b], four[b]) >= 1e-3
        assert R.one_minus_cos(three[b], four[b]) >= 1e-3 or b >= 6
    assert R.one_minus_cos(three[6], alone[6]) <= 1e-15  # frame 6 is alone in its group of 3


def test_encoder_floors_are_below_the_bar():
    """The bar of the GPU encoder test (1 - cos <= 1e-9) leaves room above both floors."""
    _, e_f32, e_split = R.encoder_reference(7, 3)
    print(f"e_f32 {e_f32:.3e}, e_split {e_split:.3e}")
    assert e_f32 < 1e-9 and e_split < 1e-9


# ------------------------------------------------------------------ packer against the table
def _packed():
    from mlgate.crica import pack_head
    return pack_head(R.head_sd(), CPU)


def test_pack_head_against_the_weight_table():
    w, p = _packed()
    assert len(w) == 24 and p == 3.0
    check = lambda lst: _native.ops().weights_check("crica", lst)  # noqa: E731
    check(w)
    bad = list(w)
    assert bad[6].dtype == torch.bfloat16
    bad[6] = bad[6].float()
    with pytest.raises(RuntimeError, match=re.escape("weights[6] (layers[0].fc1_w)") + ".*bf16.*got f32"):
        check(bad)
    bad = list(w)
    bad[23] = bad[23][:-1]
    with pytest.raises(RuntimeError, match=re.escape("weights[23] (layers[1].ln2_b)") + ".*got 767 elements"):
        check(bad)
    with pytest.raises(RuntimeError, match="expected 24 tensors, got 23"):
        check(w[:-1])
    assert tuple(w[0].shape) == (2304, 1536) and tuple(w[20].shape) == (768, 4096)


# ------------------------------------------------------------------ checkpoint loader
def _checkpoint(tmp_path, name, wrap=None, prefix="", extra=None):
    sd = {prefix + k: torch.from_numpy(np.asarray(v)) for k, v in W.crica_state_dict(0).items()}
    sd.update(extra or {})
    path = tmp_path / name
    torch.save({wrap: sd} if wrap else sd, path)
    return str(path)


def test_checkpoint_loader(tmp_path, monkeypatch):
    want = W.crica_state_dict(0)
    for i, (wrap, prefix) in enumerate([(None, ""), ("model_state_dict", "module."), ("state_dict", "")]):
        got = W.load_crica_state_dict(_checkpoint(tmp_path, f"c{i}.pth", wrap, prefix))
        assert sorted(got) == sorted(W.crica_keys())
        assert all(np.array_equal(got[k], want[k]) for k in want)
    extra = {"backbone.blocks.3.adapter1.D_fc1.weight": torch.zeros(4, 4),
             "backbone.blocks.3.adapter1.D_fc1.bias": torch.zeros(4), "backbone.mask_token": torch.zeros(1, 768),
             "encoder_layer.linear1.bias": torch.zeros(2048)}
    path = _checkpoint(tmp_path, "adapters.pth", "model_state_dict", "module.", extra)
    with pytest.raises(ValueError, match=r"2 backbone tensors.*'backbone\.blocks\.3\.adapter1\.D_fc1\.weight'"):
        W.load_crica_state_dict(path)
    monkeypatch.setenv("MLGATE_CRICAVPR_WEIGHTS", path)
    with pytest.raises(ValueError, match="adapter"):
        W.resolve_crica_state_dict()
    monkeypatch.delenv("MLGATE_CRICAVPR_WEIGHTS")
    assert W.resolve_crica_state_dict()[1].startswith("synthetic")
    assert float(W.crica_state_dict(0)["aggregation.1.p"][0]) == 3.0


# ------------------------------------------------------------------ the C ABI's argument checks
EINVAL, ENOMEM = -1, -3
P = ctypes.c_void_p
VIT_FIELDS = ([("struct_size", ctypes.c_uint32), ("abi_version", ctypes.c_uint32)] +
              [(f"p{i}", P) for i in range(4 + 12 * 14 + 2)] + [("packing", ctypes.c_int)])
CRICA_FIELDS = ([("struct_size", ctypes.c_uint32), ("abi_version", ctypes.c_uint32), ("gem_p", ctypes.c_float)] +
                [(f"p{i}", P) for i in range(24)])
VitWeights = type("VitWeights", (ctypes.Structure,), {"_fields_": VIT_FIELDS})
CricaWeights = type("CricaWeights", (ctypes.Structure,), {"_fields_": CRICA_FIELDS})


class Abi:
    """Dummy pointers (256-byte aligned, never dereferenced: every check precedes the first GPU
    call) and well-formed structs; call(...) runs mlg_crica_forward with one argument changed."""

    def __init__(self):
        self.L = _native.lib()
        self._buf = ctypes.create_string_buffer(1 << 16)
        self.d = (ctypes.addressof(self._buf) + 255) & ~255
        self.vit, self.cw = VitWeights(), CricaWeights()
        for s, cls in ((self.vit, VitWeights), (self.cw, CricaWeights)):
            s.struct_size, s.abi_version = ctypes.sizeof(cls), 3
            for name, typ in cls._fields_:
                if typ is P:
                    setattr(s, name, self.d)
        self.vit.packing, self.cw.gem_p = 4, 3.0
        self.need = self.L.mlg_vit_workspace_bytes(2, 322)

    def forward(self, B=2, image_size=322, flags=4, group=1, ws_bytes=None, desc=None, local=None, ws=None):
        return self.L.mlg_crica_forward(ctypes.byref(self.vit), ctypes.byref(self.cw), self.d, B, 480, 640, 3,
                                        480 * 640 * 3, image_size, flags, group, self.d if ws is None else ws,
                                        self.need if ws_bytes is None else ws_bytes, self.d if desc is None else desc,
                                        local, None)

    def encoder(self, B=2, group=1, ws_bytes=None, pooled=None):
        need = 2 * 14 * 26624 + 16384 if ws_bytes is None else ws_bytes  # MLG_CRICA_HEAD_WS_BYTES(2)
        return self.L.mlg_op_crica_encoder(ctypes.byref(self.cw), self.d if pooled is None else pooled, B, group,
                                           self.d, need, self.d, None)


def test_struct_layout_matches_the_header():
    assert ctypes.sizeof(CricaWeights) == 16 + 24 * 8 and CricaWeights.p0.offset == 16


def test_abi_refuses_bad_arguments_before_any_gpu_call():
    a = Abi()
    assert a.need > 0
    # a short workspace is the only thing wrong: every other check has passed by then
    assert a.forward(ws_bytes=a.need - 1) == ENOMEM
    assert a.encoder(ws_bytes=2 * 14 * 26624) == ENOMEM
    for kw in ({"group": 0}, {"group": 33}, {"B": 0}, {"B": 4097}, {"image_size": 154}, {"image_size": 323},
               {"flags": 0}, {"desc": a.d + 4}, {"local": a.d + 8}, {"ws": a.d + 4}):
        assert a.forward(ws_bytes=a.need - 1, **kw) == EINVAL, kw
    for kw in ({"group": 0}, {"group": 33}, {"B": 0}, {"B": 4097}, {"pooled": a.d + 4}):
        assert a.encoder(ws_bytes=0, **kw) == EINVAL, kw
    for p in (0.0, -1.0, float("nan"), float("inf")):
        a.cw.gem_p = p
        assert a.forward(ws_bytes=a.need - 1) == EINVAL and a.encoder(ws_bytes=0) == EINVAL, p
    a.cw.gem_p = 3.0
    for field, value in (("p7", 0), ("p0", a.d + 2)):  # a null and a misaligned weight pointer
        setattr(a.cw, field, value)
        assert a.forward(ws_bytes=a.need - 1) == EINVAL and a.encoder(ws_bytes=0) == EINVAL, field
        setattr(a.cw, field, a.d)
    for size, version in ((ctypes.sizeof(CricaWeights) - 8, 3), (ctypes.sizeof(CricaWeights), 2)):  # foreign heads
        a.cw.struct_size, a.cw.abi_version = size, version
        assert a.forward(ws_bytes=a.need - 1) == EINVAL and a.encoder(ws_bytes=0) == EINVAL
    a.cw.struct_size, a.cw.abi_version = ctypes.sizeof(CricaWeights), 3
    a.vit.packing = 0  # plain-bf16 trunk weights under the split flag
    assert a.forward(ws_bytes=a.need - 1) == EINVAL
    a.vit.packing = 4
    assert a.L.mlg_op_crica_pool(a.d, a.d, a.d, 1, 11, ctypes.c_float(3.0), a.d, None) == EINVAL
    assert a.L.mlg_op_crica_pool(a.d, a.d, a.d, 1, 23, ctypes.c_float(0.0), a.d, None) == EINVAL
    assert a.L.mlg_op_crica_pool(a.d, None, a.d, 1, 23, ctypes.c_float(3.0), a.d, None) == EINVAL
    assert a.forward(ws_bytes=a.need - 1) == ENOMEM  # the structs are whole again


def test_head_workspace_macro_covers_the_carve():
    """MLG_CRICA_HEAD_WS_BYTES(B) is sufficient: one byte less than the six 256-byte-aligned
    buffers is refused, the macro's value is not (checked at the sizes where rounding is worst)."""
    a = Abi()
    for B in (1, 2, 3, 37, 4096):
        M = 14 * B
        carve = sum((n + 255) // 256 * 256 for n in (M * 3072, M * 3072, M * 9216, M * 3072, M * 8192, 9216))
        assert carve <= B * 14 * 26624 + 16384
        assert a.encoder(B=B, ws_bytes=carve - 1) == ENOMEM


# ------------------------------------------------------------------ the drop-in
def test_native_rejects_other_dimensions_and_backbones(monkeypatch):
    monkeypatch.delenv("MLGATE_CRICAVPR_NATIVE", raising=False)
    img = np.zeros((32, 32, 3), np.uint8)
    for kw, names in (({"descriptor_dim": 768}, ("10752", "768")), ({"backbone": "dinov2_vitl14"}, ("dinov2_vitl14",))):
        m = CricaVPR(**kw)
        m.native = True
        for call in (lambda: m.extract_descriptor(img), lambda: m.extract_descriptors([img]),
                     lambda: m.add_image(img, 0.0), lambda: m.add_images([img], [0.0])):
            with pytest.raises(ValueError) as e:
                call()
            assert all(n in str(e.value) for n in names), str(e.value)
    monkeypatch.setenv("MLGATE_CRICAVPR_NATIVE", "1")
    env = CricaVPR(descriptor_dim=768)
    assert env.native is None and env.cross_image_group == 1
    with pytest.raises(ValueError):
        env.extract_descriptor(img)
    m = CricaVPR()
    m.native, m.cross_image_group = True, 33
    with pytest.raises(ValueError, match="group"):
        m.extract_descriptor(img)


def test_default_never_imports_the_native_engine(monkeypatch):
    monkeypatch.delenv("MLGATE_CRICAVPR_NATIVE", raising=False)
    sys.modules.pop("mlgate.crica", None)
    m = CricaVPR()
    assert m._native_engine() is None and m.native is None
    assert "mlgate.crica" not in sys.modules
