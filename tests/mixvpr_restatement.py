"""fp32 restatement of MixVPR's native model (test infrastructure only): the published
amaralibey/MixVPR MixVPRModel(backbone='resnet50', out_dim=4096) that
``MixVPR._load_model`` builds (scripts/semantic_gating/place_recognition.py:227-239) and
``_preprocess`` feeds (:308-332), in torch on the CPU, in the reference's own order
(channel_proj on [B, 1024, 400], then row_proj).

  preprocess : oracle.vit.preprocess(image, 320, swap_rb=True)
  trunk      : torchvision resnet50 through layer3 (eval BatchNorm) -> [B, 1024, 20, 20]
  aggregator : 4 x (x + Linear2(ReLU(Linear1(LayerNorm400(x))))) on x.flatten(2),
               channel_proj over the channel axis, row_proj, flatten, L2 normalise.

``head`` can omit single terms (the sensitivity test) and can round every operand of the
four GEMMs a bf16 MFMA kernel runs (LayerNorm output, Linear1 weight, ReLU output, Linear2
weight) to bf16, which gives the operand-rounding floor the GPU bar is a multiple of.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import resnet as ors
from oracle import vit as ovit

HW, C, DEPTH, ROWS = 400, 1024, 4, 4
OMITTABLE = tuple(f"block{i}" for i in range(DEPTH)) + ("b1", "b2", "ln_affine", "channel_bias", "row_bias")


def _agg(sd, dtype):
    return {k[len("aggregator."):]: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items()
            if k.startswith("aggregator.")}


def _bf(t):
    return t.bfloat16().to(t.dtype)


def head(sd, feat, omit=None, bf16_operands=False, dtype=torch.float32):
    """feat [B, 1024, 400] (layer3 output, flattened) -> descriptors [B, 4096]."""
    a = _agg(sd, dtype)
    x = torch.as_tensor(feat).to(dtype)
    rnd = _bf if bf16_operands else (lambda t: t)
    with torch.no_grad():
        for i in range(DEPTH):
            if omit == f"block{i}":
                continue
            p = f"mix.{i}.mix."
            g, b = (None, None) if omit == "ln_affine" else (a[p + "0.weight"], a[p + "0.bias"])
            t = F.layer_norm(x, (HW,), g, b, eps=1e-5)
            h = rnd(t) @ rnd(a[p + "1.weight"]).T
            if omit != "b1":
                h = h + a[p + "1.bias"]
            y = rnd(F.relu(h)) @ rnd(a[p + "3.weight"]).T
            if omit != "b2":
                y = y + a[p + "3.bias"]
            x = x + y
        x = F.linear(x.permute(0, 2, 1), a["channel_proj.weight"],
                     None if omit == "channel_bias" else a["channel_proj.bias"]).permute(0, 2, 1)
        x = F.linear(x, a["row_proj.weight"], None if omit == "row_bias" else a["row_proj.bias"])
        return F.normalize(x.flatten(1), p=2, dim=-1)


def trunk(sd, x):
    """torchvision resnet50 children up to layer3 on x [B, 3, 320, 320] -> [B, 1024, 20, 20]."""
    w = {k[len("backbone.model."):]: torch.as_tensor(np.asarray(v, np.float32)) for k, v in sd.items()
         if k.startswith("backbone.model.")}
    with torch.no_grad():
        x = F.relu(ors._bn(F.conv2d(x, w["conv1.weight"], stride=2, padding=3), w, "bn1"))
        x = F.max_pool2d(x, 3, 2, 1)
        for li, (width, blocks, stride) in enumerate(ors.STAGES[:3], 1):
            for b in range(blocks):
                p = f"layer{li}.{b}"
                s = stride if b == 0 else 1
                idt = x
                y = F.relu(ors._bn(F.conv2d(x, w[p + ".conv1.weight"]), w, p + ".bn1"))
                y = F.relu(ors._bn(F.conv2d(y, w[p + ".conv2.weight"], stride=s, padding=1), w, p + ".bn2"))
                y = ors._bn(F.conv2d(y, w[p + ".conv3.weight"]), w, p + ".bn3")
                if b == 0:
                    idt = ors._bn(F.conv2d(x, w[p + ".downsample.0.weight"], stride=s), w, p + ".downsample.1")
                x = F.relu(y + idt)
    return x


def preprocess(image):
    """MixVPR._preprocess -> float32 [1, 3, 320, 320]."""
    return ovit.preprocess(image, 320, swap_rb=True)


def descriptor(sd, images):
    """The whole model on a list of uint8 images -> float32 [B, 4096]."""
    x = torch.cat([preprocess(im) for im in images])
    return head(sd, trunk(sd, x).flatten(2))


def one_minus_cos(a, b):
    """Row-wise 1 - cos in float64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 1.0 - (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


# ------------------------------------------------------------ shared head inputs
HEAD_SEED, HEAD_BATCH = 5, 17  # 17 images = 17,408 rows: more 64-row tiles than the chip has CUs


@functools.lru_cache(maxsize=None)
def head_features():
    """Seeded post-ReLU layer3-like features [17, 1024, 400] float32 with a per-channel scale
    spread of e^-1 .. e^1 (shared by the CPU and GPU head tests: do not write to it)."""
    rng = np.random.default_rng(HEAD_SEED)
    scale = np.exp(rng.uniform(-1.0, 1.0, (1, C, 1))).astype(np.float32)
    f = np.maximum(rng.standard_normal((HEAD_BATCH, C, HW), dtype=np.float32), 0) * scale
    return f


@functools.lru_cache(maxsize=None)
def head_weights():
    from mlgate.weights import mixvpr_state_dict
    return mixvpr_state_dict(0)


@functools.lru_cache(maxsize=None)
def head_reference(n=HEAD_BATCH):
    """(fp32 restatement [n, 4096], e_emul [n]) on the first n shared feature images; e_emul =
    1 - cos between the restatement with bf16-rounded GEMM operands and the fp32 one."""
    f = torch.from_numpy(head_features()[:n])
    ref = head(head_weights(), f).numpy()
    emul = head(head_weights(), f, bf16_operands=True).numpy()
    ref.setflags(write=False)
    return ref, one_minus_cos(emul, ref)
