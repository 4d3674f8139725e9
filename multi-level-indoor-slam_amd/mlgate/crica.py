"""CricaVPR descriptor engine on the mlgate HIP kernels (the native branch of ``CricaVPR``).

Reference: ``CricaVPR`` (place_recognition.py:508-803) declares ``descriptor_dim=10752`` and
"cross-image correlation-aware representation learning", then always falls back to
DINOv2 + GeM, 768-dim (:558-578: ``from cricavpr import ...`` never succeeds).
``mlgate.vpr.CricaVPR`` keeps that fallback by default; this engine is the descriptor the
class names, opt-in (``MLGATE_CRICAVPR_NATIVE=1``), like the other three native branches.

Per call: the split-bf16 ViT-B/14 forward at 322 x 322 with the R/B swap (the forward the
fallback runs), then upstream CricaVPRNet's head on its final-normed tokens (csrc/crica.hip):
14 rows of 768 per frame -- the CLS token and the GeM of 2 x 2 and 3 x 3 regions of the
L2-normalised patch tokens -- a 2-layer transformer encoder whose sequence axis is the
images of a group, and one L2 normalisation of the 10752 values.

Groups.  A descriptor must not depend on how a call happens to be batched, so the images
that attend to each other are named: frames [j G, (j + 1) G) of a call form group j (the
last may be short), G = ``group`` (1 .. 32, default 1: each frame alone, what the reference's
one-image-per-call ``extract_global_descriptor`` would compute).  A group's descriptors are
bit-identical whatever else is in the call; ``forward`` chunks by ``max_batch`` on group
boundaries.
"""
import numpy as np
import torch

from . import _native
from .vit import VitB14, split_weight
from .weights import CRICA_DIM, CRICA_LAYERS, CRICA_ROWS, EMBED, given_or_resolved, sub_state_dict

IMAGE_SIZE = 322
MAX_GROUP = 32  # include/mlgate.h MLG_CRICA_MAX_GROUP
# mlg_crica_layer field order and the nn.TransformerEncoderLayer tensor behind each
LAYER_ORDER = (("in_w", "self_attn.in_proj_weight"), ("in_b", "self_attn.in_proj_bias"),
               ("out_w", "self_attn.out_proj.weight"), ("out_b", "self_attn.out_proj.bias"),
               ("ln1_g", "norm1.weight"), ("ln1_b", "norm1.bias"),
               ("fc1_w", "linear1.weight"), ("fc1_b", "linear1.bias"),
               ("fc2_w", "linear2.weight"), ("fc2_b", "linear2.bias"),
               ("ln2_g", "norm2.weight"), ("ln2_b", "norm2.bias"))


def pack_head(sd, device):
    """(the ``head`` list of torch.ops.mlgate.crica_forward / crica_encoder on ``device``,
    gem_p): per layer LAYER_ORDER, the GEMM weights bf16 [out, 2 in] = [W_hi | W_lo]."""
    w = []
    for i in range(CRICA_LAYERS):
        for field, key in LAYER_ORDER:
            t = torch.as_tensor(np.asarray(sd[f"encoder.layers.{i}.{key}"], np.float32)).to(device)
            w.append(split_weight(t) if field.endswith("_w") else t.contiguous())
    return w, float(np.asarray(sd["aggregation.1.p"], np.float32).reshape(-1)[0])


def check_group(group):
    group = int(group)
    if not 1 <= group <= MAX_GROUP:
        raise ValueError(f"group must be in 1..{MAX_GROUP}, got {group}")
    return group


class CricaGPU:
    """Packed ViT-B/14 trunk + CricaVPR head for batched 10752-dim descriptor extraction."""

    def __init__(self, state_dict=None, device="cuda", image_size=IMAGE_SIZE, max_batch=64, group=1,
                 pretrained_path=None):
        state_dict, self.weights_source = given_or_resolved("crica", state_dict, pretrained_path)
        self.group = check_group(group)
        if max_batch < self.group:
            raise ValueError(f"max_batch = {max_batch} does not hold one group of {self.group}")
        self._vit = VitB14(sub_state_dict(state_dict, "backbone."), device=device, image_size=image_size,
                           max_batch=max_batch, pool="gem", swap_rb=True, precise=True)
        if self._vit.grid < 12:
            raise ValueError("image_size must be at least 168 (a 12 x 12 patch grid)")
        self.device = self._vit.device
        self.image_size, self.max_batch = image_size, max_batch
        self.n_local = self._vit.n_local
        self.descriptor_dim = CRICA_DIM
        self._head, self.gem_p = pack_head(state_dict, self.device)

    def forward(self, frames, with_local=False):
        """frames: uint8 [B, H, W, C] (or [B, H, W]) device tensor -> float32 [B, 10752]
        (and, from the same forward, the local features [B, n_local, 768] that
        ``VitB14.forward(frames, with_local=True)`` returns)."""
        desc, local = _native.ops().crica_forward(_native.device_frames(frames), self._vit._w, self._head, self.gem_p,
                                                  self.image_size, self._vit.flags, self.group, self.max_batch,
                                                  bool(with_local))
        return (desc, local) if with_local else desc

    def trunk(self, frames):
        """The trunk's residual stream before the final LayerNorm: float32 [B, 1 + g^2, 768]."""
        return _native.ops().vit_trunk(_native.device_frames(frames), self._vit._w, self.image_size, self._vit.flags,
                                       self.max_batch)

    def pool(self, tokens_prenorm):
        """The pyramid alone: float32 [B, 1 + g^2, 768] device tokens -> [B, 14, 768]."""
        return _native.ops().crica_pool(tokens_prenorm.contiguous(), self._vit._w[-2], self._vit._w[-1], self.gem_p)

    def encode(self, pooled, group=None):
        """The encoder and the final normalisation alone: float32 [B, 14, 768] -> [B, 10752]."""
        if pooled.dim() != 3 or pooled.shape[1:] != (CRICA_ROWS, EMBED):
            raise ValueError(f"pooled must be [B, {CRICA_ROWS}, {EMBED}]")
        group = self.group if group is None else check_group(group)
        return _native.ops().crica_encoder(pooled.contiguous(), self._head, self.gem_p, group)
