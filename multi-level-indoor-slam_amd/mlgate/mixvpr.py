"""MixVPR descriptor engine on the mlgate HIP kernels (the native branch of ``MixVPR``).

Reference: ``MixVPR._load_model`` / ``extract_descriptor`` / ``_preprocess``
(place_recognition.py:227-239, 308-332).  The reference builds
``MixVPRModel(backbone='resnet50', out_dim=4096)`` (amaralibey/MixVPR: torchvision
resnet50 cropped after layer3 + the feature-mixer aggregator) when the ``mixvpr`` package
imports, else falls back to a ResNet-50 GAP; the package is absent wherever the reference
runs, so ``mlgate.vpr.MixVPR`` keeps the fallback by default and this engine is opt-in
(``MLGATE_MIXVPR_NATIVE=1``), like SALAD's native branch.

Per batch of frames: preprocessing (cv2 INTER_LINEAR to 320 x 320, BGR -> RGB, ImageNet
normalisation), the cropped trunk (csrc/resnet.hip at side 320 -> [B, 400, 1024] f32),
then the fused head (csrc/mixvpr.hip): 4 mixer blocks + row_proj per 64-row tile in one
kernel, channel_proj + L2 normalisation in a second.  Output float32 [B, 4096].
"""
import numpy as np
import torch

from . import _native
from .lightglue import pack_kstep
from .resnet import pack_trunk
from .weights import (MIXVPR_CHANNELS, MIXVPR_DEPTH, MIXVPR_HW, MIXVPR_ROWS, MIXVPR_STAGES, given_or_resolved,
                      sub_state_dict)

IMAGE_SIZE = 320
DESC_DIM = MIXVPR_CHANNELS * MIXVPR_ROWS
NPAD, PPAD = 416, 512  # packed rows / columns of a Linear(400, 400); length of a per-feature vector


def pack_head(sd):
    """amaralibey/MixVPR aggregator tensors -> the 7 float32 arrays of mlg_mixvpr_weights'
    head (include/mlgate.h), in order: mix_w [4][2][26][416][16] (bf16 on the device),
    mix_p [4][4][512], row_w [4][512], chan_w [1024][1024], chan_b [1024], row_s [4], row_b [4].

    The kernels apply row_proj before channel_proj:
    out[o, r] = sum_c Wc[o, c] P[c, r] + bc[o] s[r] + br[r], P = x Wr^T, s[r] = sum_i Wr[r, i]."""
    a = "aggregator."
    g = lambda k: np.asarray(sd[a + k], np.float32)  # noqa: E731
    hw = MIXVPR_HW
    mix_w = np.zeros((MIXVPR_DEPTH, 2, NPAD // 16, NPAD, 16), np.float32)
    mix_p = np.zeros((MIXVPR_DEPTH, 4, PPAD), np.float32)
    for i in range(MIXVPR_DEPTH):
        p = f"mix.{i}.mix."
        for j, lin in enumerate(("1", "3")):
            w = np.zeros((NPAD, NPAD), np.float32)
            w[:hw, :hw] = g(p + lin + ".weight")
            mix_w[i, j] = pack_kstep(w)
        for j, k in enumerate(("0.weight", "0.bias", "1.bias", "3.bias")):
            mix_p[i, j, :hw] = g(p + k)
    row_w = np.zeros((MIXVPR_ROWS, PPAD), np.float32)
    row_w[:, :hw] = g("row_proj.weight")
    row_s = g("row_proj.weight").astype(np.float64).sum(axis=1).astype(np.float32)
    return [mix_w, mix_p, row_w, np.ascontiguousarray(g("channel_proj.weight")), g("channel_proj.bias"), row_s,
            g("row_proj.bias")]


def head_list(sd, device):
    """The torch.ops.mlgate.mixvpr_* ``head`` list on ``device`` (pack_head; mix_w in bf16)."""
    return [torch.as_tensor(t).to(device, torch.bfloat16 if i == 0 else torch.float32).contiguous()
            for i, t in enumerate(pack_head(sd))]


class MixVprGPU:
    """Packed device weights for batched MixVPR descriptor extraction."""

    def __init__(self, state_dict=None, device="cuda", max_batch=32, pretrained_path=None, seed=0):
        self.device = _native.require_device(device)
        state_dict, self.weights_source = given_or_resolved("mixvpr", state_dict, pretrained_path, seed)
        self.max_batch = max_batch
        self._trunk = pack_trunk(sub_state_dict(state_dict, "backbone.model."), self.device, MIXVPR_STAGES)
        self._head = head_list(state_dict, self.device)

    def forward(self, frames):
        """frames: uint8 [B, H, W, C] (or [B, H, W]) device tensor -> float32 [B, 4096]."""
        return _native.ops().mixvpr_forward(_native.device_frames(frames), self._trunk, self._head, self.max_batch)

    def head(self, features):
        """features: float32 [B, 400, 1024] device tensor (layer3 output, NHWC) -> float32 [B, 4096]."""
        return _native.ops().mixvpr_head(features.contiguous(), self._head)

    def preprocess(self, frames):
        """frames: uint8 [B, H, W, C] device tensor -> float32 [B, 320, 320, 3] (RGB, normalised)."""
        if frames.dim() == 3:
            frames = frames.unsqueeze(-1)
        return _native.ops().mixvpr_preprocess(frames.contiguous())
