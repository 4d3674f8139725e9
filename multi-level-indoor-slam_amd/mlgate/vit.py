"""DINOv2 ViT-S/B/L-14 + GeM descriptor engine (CricaVPR path) on the mlgate HIP kernels.

Device-resident replacement for what CricaVPR does per keyframe
(place_recognition.py:613-667, 759-803): preprocessing, the hub
``get_intermediate_layers`` forward, GeM pooling and the local-feature cache -- all
from ONE forward (the reference runs the identical forward twice per add_image, once
for the descriptor and once for the local features).  Frames go in as uint8
[B, H, W, C] device tensors; everything up to the float32 descriptors stays in HBM.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import _native
from .weights import DEFAULT_BACKBONE, EMBED, PATCH, backbone_config, check_state_dict

PATCH_K = 768  # 3*14*14 = 588 patch inputs zero-padded to 12 K-tiles of 64 (include/mlgate.h)
BLOCK_ORDER = ("norm1_w", "norm1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ls1", "norm2_w", "norm2_b", "fc1_w",
               "fc1_b", "fc2_w", "fc2_b", "ls2")  # mlg_vit_block field order
BF16_FIELDS = {"qkv_w", "proj_w", "fc1_w", "fc2_w"}  # GEMM weights; everything else float32


def resample_pos_embed(pos_embed, grid):
    """Hub DinoVisionTransformer.interpolate_pos_encoding (square input): bicubic,
    scale_factor (grid + 0.1) / 37, antialias off.  One-time weight transform."""
    pos_embed = pos_embed.float()
    m = int(math.sqrt(pos_embed.shape[1] - 1))
    if grid == m:
        return pos_embed
    s = float(grid + 0.1) / m
    patch = pos_embed[:, 1:].reshape(1, m, m, -1).permute(0, 3, 1, 2)
    patch = F.interpolate(patch, mode="bicubic", antialias=False, scale_factor=(s, s))
    patch = patch.permute(0, 2, 3, 1).reshape(1, grid * grid, -1)
    return torch.cat((pos_embed[:, :1], patch), dim=1).contiguous()


MLG_VIT_SPLIT = 4  # include/mlgate.h


def split_weight(w):
    """[out, in] float32 -> bf16 [out, 2 in] = [W_hi | W_lo] (MLG_VIT_SPLIT packing:
    hi = bf16(W), lo = bf16(W - hi), so W = hi + lo to 2^-17)."""
    w = w.to(torch.float32)
    hi = w.to(torch.bfloat16)
    lo = (w - hi.to(torch.float32)).to(torch.bfloat16)
    return torch.cat([hi, lo], dim=1).contiguous()


def pack_weights(sd, device, grid, precise, backbone=DEFAULT_BACKBONE):
    """The torch.ops.mlgate.vit_forward_into / dino_forward_into weight list on ``device``:
    patch_w, patch_b, cls, pos (resampled to ``grid`` x ``grid`` patches), depth x BLOCK_ORDER,
    norm_w, norm_b; the GEMM weights bf16, [W_hi | W_lo] with ``precise``.  The split GEMM
    runs 256-column tiles, so with ``precise`` a GEMM weight whose row count is no multiple of
    256 (ViT-S: patch, qkv, proj, fc2) gets zero rows up to the next one (include/mlgate.h)."""
    f32, bf = torch.float32, torch.bfloat16
    embed, depth = backbone_config(backbone)[:2]

    def dev(a, dtype):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(device, torch.float32).to(dtype).contiguous()

    def gemm_w(a):  # a GEMM weight in the layout of this forward
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        t = t.to(device, torch.float32)
        if not precise:
            return t.to(bf).contiguous()
        return split_weight(F.pad(t, (0, 0, 0, -t.shape[0] % 256)))

    pw = torch.as_tensor(np.asarray(sd["patch_embed.proj.weight"], np.float32)).reshape(embed, -1)
    pos = torch.as_tensor(np.asarray(sd["pos_embed"], np.float32)).to(device)
    w = [gemm_w(F.pad(pw, (0, PATCH_K - pw.shape[1]))), dev(sd["patch_embed.proj.bias"], f32),
         dev(np.asarray(sd["cls_token"], np.float32).reshape(embed), f32),
         dev(resample_pos_embed(pos, grid).reshape(-1, embed), f32)]
    names = {"norm1_w": "norm1.weight", "norm1_b": "norm1.bias", "qkv_w": "attn.qkv.weight",
             "qkv_b": "attn.qkv.bias", "proj_w": "attn.proj.weight", "proj_b": "attn.proj.bias",
             "ls1": "ls1.gamma", "norm2_w": "norm2.weight", "norm2_b": "norm2.bias", "fc1_w": "mlp.fc1.weight",
             "fc1_b": "mlp.fc1.bias", "fc2_w": "mlp.fc2.weight", "fc2_b": "mlp.fc2.bias", "ls2": "ls2.gamma"}
    for i in range(depth):
        for f in BLOCK_ORDER:
            v = sd[f"blocks.{i}." + names[f]]
            w.append(gemm_w(v) if f in BF16_FIELDS else dev(v, f32))
    w += [dev(sd["norm.weight"], f32), dev(sd["norm.bias"], f32)]
    return w


class VitB14:
    """Packed device weights + workspace for batched CricaVPR descriptor extraction.

    precise=True selects the split-bf16 forward (MLG_VIT_SPLIT, include/mlgate.h): every
    GEMM and attention operand carried as a hi + lo bf16 pair, three MFMA products each.
    Descriptors then agree with the fp32 network to ~1e-11 (1 - cos) instead of ~1e-5, and
    kNN rankings over near-identical descriptors follow the fp32 reference's
    (tests/test_bench_parity_gpu.py).  It is the default everywhere the descriptors feed
    retrieval (DeviceGate, the CricaVPR / AnyLoc drop-ins); precise=False keeps the plain
    bf16 forward (3x fewer MFMA products; SALAD's trunk, A/B tools)."""

    backbone, embed = DEFAULT_BACKBONE, EMBED  # DinoVit: the instance's

    def __init__(self, state_dict, device="cuda", image_size=322, max_batch=64, pool="gem", swap_rb=True,
                 precise=True):
        self.device = _native.require_device(device)
        if image_size % PATCH:
            raise ValueError("image_size must be a multiple of 14")
        self.image_size, self.grid = image_size, image_size // PATCH
        self.n_patches = self.grid * self.grid
        self.n_local = self.n_patches - 1  # tokens 2.. of get_intermediate_layers (CLS + patch 0 dropped)
        self.max_batch = max_batch
        self.precise = bool(precise)
        self.flags = ((1 if pool == "mean" else 0) | (0 if swap_rb else 2)  # MLG_VIT_POOL_MEAN / KEEP_CHANNELS
                      | (MLG_VIT_SPLIT if self.precise else 0))
        self._w = pack_weights(state_dict, self.device, self.grid, self.precise, self.backbone)

    def _op(self, frames, *rest):
        """The forward operator on this engine's weights: all a subclass chooses."""
        _native.ops().vit_forward_into(frames, self._w, *rest)

    # ------------------------------------------------------------ forward
    def forward_into(self, frames, desc_out, local_out=None):
        """frames: uint8 [B, H, W, C] device tensor (C = 1, 3 BGR or 4 BGRA; or [B, H, W]).
        Writes float32 descriptors [B, embed] (and local features [B, n_local, embed]) on the
        current stream: torch.ops.mlgate.vit_forward_into (DinoVit: dino_forward_into)."""
        self._op(_native.device_frames(frames), self.image_size, self.flags, self.max_batch, desc_out, local_out)

    def forward(self, frames, with_local=False):
        B = frames.shape[0]
        desc = torch.empty(B, self.embed, dtype=torch.float32, device=self.device)
        local = (torch.empty(B, self.n_local, self.embed, dtype=torch.float32, device=self.device)
                 if with_local else None)
        self.forward_into(frames, desc, local)
        return (desc, local) if with_local else desc


class DinoVit(VitB14):
    """VitB14 for any of the three hub backbones (weights.BACKBONES): dinov2_vits14 (384 wide),
    dinov2_vitb14 (768) or dinov2_vitl14 (1024, 24 blocks), through mlg_dino_forward.  Same
    arguments, flags and outputs with 768 read as ``embed``; ``state_dict`` must be that
    backbone's (a checkpoint of another width is refused, naming the first tensor that
    disagrees).  At dinov2_vitb14 it launches the kernels VitB14 launches: the same bits."""

    def __init__(self, state_dict, backbone=DEFAULT_BACKBONE, **kwargs):
        self.backbone = backbone
        self.embed, self.depth, self.heads, _ = backbone_config(backbone)
        check_state_dict(state_dict, backbone)
        super().__init__(state_dict, **kwargs)

    def _op(self, frames, *rest):
        _native.ops().dino_forward_into(frames, self._w, self.embed, *rest)


def engine_for(state_dict, backbone=DEFAULT_BACKBONE, **kwargs):
    """The engine of ``backbone``: VitB14 for dinov2_vitb14, DinoVit otherwise.  DinoVit at
    dinov2_vitb14 gives the same bits, but ViT-B keeps its own entry point (vit_forward_into,
    mlg_vit_forward over the inline mlg_vit_weights): it is the ABI that existing callers link
    against, and tests/test_dino_backbones_gpu.py compares the two entry points bit for bit,
    so the default pipeline must go on running the first."""
    if backbone == DEFAULT_BACKBONE:
        return VitB14(state_dict, **kwargs)
    return DinoVit(state_dict, backbone=backbone, **kwargs)
