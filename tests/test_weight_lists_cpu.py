"""The Python weight packers against the C++ weight tables (csrc/weight_tables.h), on the CPU.

Each model's seeded synthetic state dict is packed on the CPU device by the function the GPU
engine packs with and handed to ``torch.ops.mlgate.weights_check``, which runs the checks the
model's operator applies to its list (length, and per tensor: one device, contiguous, element
kind, element count, bf16 alignment) without launching anything.  A packer and a table that
drift apart (order, a dtype, a padded size) fail here; so does a corrupted list, with an error
that names the slot's index and field."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-level-indoor-slam_amd"))

from mlgate import _native, lightglue, loftr, mixvpr, resnet, salad, superglue, superpoint, vit  # noqa: E402
from mlgate import weights as W  # noqa: E402

CPU = torch.device("cpu")


def _mixvpr_trunk():
    sd = W.mixvpr_state_dict(0)
    backbone = {k[len("backbone.model."):]: v for k, v in sd.items() if k.startswith("backbone.model.")}
    return resnet.pack_trunk(backbone, CPU, W.MIXVPR_STAGES)


# model -> (packer, (bf16 slot, field), (slot cut by one row, field), list length)
MODELS = {
    "vit": (lambda: vit.pack_weights(W.synthetic_state_dict(0), CPU, 23, False),
            (6, "blocks[0].qkv_w"), (173, "norm_b"), 174),
    "vit_split": (lambda: vit.pack_weights(W.synthetic_state_dict(0), CPU, 37, True),
                  (167, "blocks[11].fc1_w"), (4, "blocks[0].norm1_w"), 174),
    "salad": (lambda: salad.aggregator_list(W.salad_state_dict(0), CPU)[0], (2, "w2"), (7, "bt2"), 8),
    "superpoint": (lambda: superpoint.weight_list(W.superpoint_state_dict(0, whiten=False), CPU),
                   (10, "w[8]"), (21, "b[8]"), 24),
    "lightglue": (lambda: lightglue.pack_weights(W.lightglue_state_dict(0), CPU),
                  (35, "self[3].Wf1"), (233, "ones"), 234),
    "superglue": (lambda: superglue.weight_list(W.superglue_state_dict(0), CPU),
                  (28, "layer[2].Wout"), (0, "kenc_w[0]"), 156),
    "resnet50": (lambda: resnet.pack_trunk(W.resnet50_state_dict(0), CPU), (32, "blocks[3].wd"), (127, "blocks[15].b3"),
                 130),
    "mixvpr_trunk": (_mixvpr_trunk, (100, "blocks[12].w2"), (1, "stem_b"), 106),
    "mixvpr_head": (lambda: mixvpr.head_list(W.mixvpr_state_dict(0), CPU), (0, "mix_w"), (6, "row_b"), 7),
    "loftr": (lambda: loftr.weight_list(W.loftr_state_dict(0, whiten=False), CPU),
              (6, "conv_w[4]"), (23, "conv_b[0]"), 129),
}
_lists = {}


def packed(model):
    """The model's list, packed once and never modified (the tests copy the list)."""
    if model not in _lists:
        _lists[model] = MODELS[model][0]()
    return list(_lists[model])


def check(model, w):
    _native.ops().weights_check(model, w)


def test_op_is_registered():
    assert "weights_check" in _native.OPS


@pytest.mark.parametrize("model", sorted(MODELS))
def test_packed_list_is_accepted(model):
    w = packed(model)
    assert len(w) == MODELS[model][3]
    check(model, w)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_float32_in_a_bf16_slot_is_refused(model):
    w = packed(model)
    i, field = MODELS[model][1]
    assert w[i].dtype == torch.bfloat16
    w[i] = w[i].float()
    with pytest.raises(RuntimeError, match=re.escape(f"weights[{i}] ({field})") + ".*bf16.*got f32"):
        check(model, w)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_short_tensor_is_refused(model):
    w = packed(model)
    i, field = MODELS[model][2]
    n = w[i].numel()
    w[i] = w[i].reshape(-1)[:-1]
    with pytest.raises(RuntimeError) as e:
        check(model, w)
    assert f"weights[{i}] ({field})" in str(e.value) and f"got {n - 1} elements" in str(e.value)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_short_list_is_refused(model):
    w = packed(model)[:-1]
    n = MODELS[model][3]
    with pytest.raises(RuntimeError, match=f"expected {n} tensors, got {n - 1}"):
        check(model, w)


def test_vit_packing_has_to_match_the_flag():
    """The MLG_VIT_SPLIT table wants every GEMM weight as [W_hi | W_lo], twice the plain size."""
    with pytest.raises(RuntimeError, match=r"weights\[0\] \(patch_w\).*got 589824 elements"):
        check("vit_split", packed("vit"))
    with pytest.raises(RuntimeError, match=r"weights\[0\] \(patch_w\).*got 1179648 elements"):
        check("vit", packed("vit_split"))


def test_strided_view_and_unknown_model_are_refused():
    w = packed("salad")
    w[1] = torch.zeros(2048)[::2]
    with pytest.raises(RuntimeError, match=r"weights\[1\] \(b1\).*non-contiguous"):
        check("salad", w)
    with pytest.raises(RuntimeError, match="unknown model"):
        check("sallad", packed("salad"))
