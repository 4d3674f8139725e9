"""The DINOv2 ViT-S / B / L-14 forward restated in float32 torch ops on the CPU, parametrised by
the backbone (tests/test_dino_backbones_cpu.py, tests/test_dino_backbones_gpu.py).

oracle/vit.py states the same network with ViT-B's shapes as module constants; this is that
forward with the width, depth and head count taken from mlgate.weights.BACKBONES:

  forward_tokens  hub ``get_intermediate_layers(x, n=1)[0]``: patch-embed conv 14 / 14, CLS
                  token, the 37 x 37 position embedding bicubic-resampled to the patch grid,
                  `depth` pre-LN blocks (LayerNorm eps 1e-6, heads of 64, qkv bias, LayerScale,
                  MLP 4 E with erf GELU), final LayerNorm, CLS stripped -> [B, (S/14)^2, E]
  gem             CricaVPR's GeM p = 3 over the tokens after the first patch
  mean_pool       AnyLoc's mean over the same tokens
  local           CricaVPR.extract_local_features: the tokens after the first patch

At dinov2_vitb14 its tokens are torch.equal to oracle.vit.forward_tokens (the same ops in the
same order); at the other widths it is pinned against transformers.Dinov2Model.  Preprocessing
is oracle.vit.preprocess, taken as it is.
"""
import numpy as np
import torch
import torch.nn.functional as F

from mlgate.weights import PATCH, backbone_config
from oracle.vit import interpolate_pos_embed, preprocess  # noqa: F401  (preprocess: re-export)


def _t(sd, k):
    v = sd[k]
    return v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))


@torch.no_grad()
def forward_tokens_with_cls(x, sd, backbone):
    """[B, 3, S, S] float32 -> [B, 1 + (S/14)^2, E], through the final LayerNorm, CLS kept."""
    E, depth, heads, _ = backbone_config(backbone)
    B, _, S, _ = x.shape
    grid = S // PATCH
    t = F.conv2d(x, _t(sd, "patch_embed.proj.weight"), _t(sd, "patch_embed.proj.bias"), stride=PATCH)
    t = t.flatten(2).transpose(1, 2)
    cls = _t(sd, "cls_token").expand(B, -1, -1)
    t = torch.cat((cls, t), dim=1)
    t = t + interpolate_pos_embed(_t(sd, "pos_embed"), grid)
    T = t.shape[1]
    hd = E // heads
    for i in range(depth):
        p = f"blocks.{i}."
        h = F.layer_norm(t, (E,), _t(sd, p + "norm1.weight"), _t(sd, p + "norm1.bias"), eps=1e-6)
        qkv = F.linear(h, _t(sd, p + "attn.qkv.weight"), _t(sd, p + "attn.qkv.bias"))
        qkv = qkv.reshape(B, T, 3, heads, hd).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0] * hd ** -0.5, qkv[1], qkv[2]
        a = (q @ k.transpose(-2, -1)).softmax(dim=-1)
        o = (a @ v).transpose(1, 2).reshape(B, T, E)
        o = F.linear(o, _t(sd, p + "attn.proj.weight"), _t(sd, p + "attn.proj.bias"))
        t = t + o * _t(sd, p + "ls1.gamma")
        h = F.layer_norm(t, (E,), _t(sd, p + "norm2.weight"), _t(sd, p + "norm2.bias"), eps=1e-6)
        h = F.gelu(F.linear(h, _t(sd, p + "mlp.fc1.weight"), _t(sd, p + "mlp.fc1.bias")))
        h = F.linear(h, _t(sd, p + "mlp.fc2.weight"), _t(sd, p + "mlp.fc2.bias"))
        t = t + h * _t(sd, p + "ls2.gamma")
    return F.layer_norm(t, (E,), _t(sd, "norm.weight"), _t(sd, "norm.bias"), eps=1e-6)


@torch.no_grad()
def forward_tokens(x, sd, backbone):
    """get_intermediate_layers(x, n=1, norm=True)[0]: [B, 3, S, S] -> [B, (S/14)^2, E]."""
    return forward_tokens_with_cls(x, sd, backbone)[:, 1:]


def local(features):
    """place_recognition.py:645-667 on forward_tokens' output: [B, (S/14)^2 - 1, E]."""
    return features[:, 1:, :]


def gem(features, p=3.0):
    """place_recognition.py:636-641 on forward_tokens' output: [B, E]."""
    return local(features).clamp(min=1e-6).pow(p).mean(dim=1).pow(1.0 / p)


def mean_pool(features):
    """AnyLoc (place_recognition.py:485) on forward_tokens' output: [B, E]."""
    return local(features).mean(dim=1)
