"""AnyLoc descriptor engine on the mlgate HIP kernels (the native branch of ``AnyLoc``).

Reference: ``AnyLoc`` (place_recognition.py:413-505) declares ``descriptor_dim=49152``,
``num_clusters=64`` and "DINOv2 + VLAD aggregation", then sets ``vlad_clusters = None``
and mean-pools the patch tokens (:484-485).  ``mlgate.vpr.AnyLoc`` keeps that mean-pool
path by default; this engine is the descriptor the class names, opt-in
(``MLGATE_ANYLOC_NATIVE=1``), like SALAD's and MixVPR's native branches.

Per batch of frames: the split-bf16 ViT-B/14 forward at 518 x 518 without a channel swap
(the tokens ``VitB14.forward(..., with_local=True)`` returns: final-normed patch tokens
with the reference's ``features[:, 1:, :]`` offset, [B, 1368, 768] f32), then hard-
assignment VLAD over a K-centre vocabulary (csrc/vlad.hip): cosine assignment on the
exact-f32 MFMA, residuals against the stored centres summed in token order, intra-
normalisation, L2 normalisation.  Output float32 [B, K * 768].

The vocabulary is fitted with ``fit_vocabulary`` (Lloyd iterations through the
``kmeans_step`` op; training tokens stay on the device) or loaded with
``load_vocabulary`` (.npy, or upstream AnyLoc's ``c_centers.pt``).
"""
import numpy as np
import torch

from . import _native
from .vit import VitB14
from .weights import EMBED, check_vocabulary, load_vocabulary  # noqa: F401  (load_vocabulary: re-export)

IMAGE_SIZE = 518
FIT_CHUNK = 16  # frames per forward while collecting training tokens


class AnyLocGPU:
    """Packed ViT-B/14 weights + a VLAD vocabulary for batched AnyLoc descriptor extraction."""

    def __init__(self, state_dict, vocabulary, device="cuda", image_size=IMAGE_SIZE, max_batch=16):
        self.device = _native.require_device(device)
        self.max_batch = max_batch
        self._vit = VitB14(state_dict, device=self.device, image_size=image_size, max_batch=max_batch, pool="mean",
                           swap_rb=False, precise=True)
        self.image_size, self.n_tokens = image_size, self._vit.n_local
        self.set_vocabulary(vocabulary)

    def set_vocabulary(self, centers):
        """centers: [K, 768] array or tensor, K a multiple of 16 in 16..128."""
        if isinstance(centers, torch.Tensor):
            centers = centers.detach().float().cpu().numpy()
        c = check_vocabulary(centers)
        self.centers = torch.from_numpy(c).to(self.device)
        self.num_clusters = c.shape[0]
        self.descriptor_dim = c.shape[0] * EMBED

    def forward(self, frames):
        """frames: uint8 [B, H, W, C] (or [B, H, W]) device tensor -> float32 [B, K * 768]."""
        return _native.ops().anyloc_forward(_native.device_frames(frames), self._vit._w, self.centers,
                                            self.image_size, self._vit.flags, self.max_batch)

    def tokens(self, frames):
        """The tokens VLAD aggregates: float32 [B, n_tokens, 768]."""
        return self._vit.forward(_native.device_frames(frames), with_local=True)[1]

    def vlad(self, tokens, with_labels=False):
        """The head alone: float32 [B, P, 768] device tokens -> [B, K * 768] (and int32 labels [B, P])."""
        desc, labels = _native.ops().vlad(tokens.contiguous(), self.centers)
        return (desc, labels) if with_labels else desc


def fit_vocabulary(tokens, num_clusters, seed=0, max_iter=100, return_info=False):
    """Spherical k-means vocabulary: centres float32 [K, 768] (a host array).

    tokens: a device float32 tensor [M, 768] (or [B, P, 768]), or a pair (engine, frames)
    of an ``AnyLocGPU`` / ``VitB14``-like object with ``tokens(frames)`` and uint8 device
    frames.  Initial centres are the unit tokens at
    ``np.random.default_rng(seed).choice(M, K, replace=False)``; Lloyd iterations run
    through ``torch.ops.mlgate.kmeans_step`` (cosine assignment, centres = means of the
    assigned unit tokens, an empty cluster keeps its centre) until no label changes or
    ``max_iter`` steps are done.  The training tokens never leave the device; one int64
    (the number of changed labels) is read back per iteration.
    return_info: also return {'labels', 'counts', 'n_iter'}."""
    if isinstance(tokens, (tuple, list)):
        engine, frames = tokens
        parts = [engine.tokens(frames[i:i + FIT_CHUNK]).reshape(-1, EMBED) for i in range(0, len(frames), FIT_CHUNK)]
        tokens = torch.cat(parts) if len(parts) > 1 else parts[0]
    if not isinstance(tokens, torch.Tensor) or tokens.device.type != "cuda" or tokens.dtype != torch.float32:
        raise TypeError("tokens must be a float32 tensor on the HIP device")
    x = tokens.reshape(-1, EMBED).contiguous()
    M, K = x.shape[0], int(num_clusters)
    if K % 16 or not 16 <= K <= 128:
        raise ValueError(f"num_clusters must be a multiple of 16 in 16..128, got {K}")
    if M < K:
        raise ValueError(f"{M} training tokens for {K} clusters")
    if max_iter < 1:
        raise ValueError("max_iter must be at least 1")
    pick = np.random.default_rng(seed).choice(M, K, replace=False)
    init = x[torch.from_numpy(pick).to(x.device)]
    centers = (init / init.norm(dim=1, keepdim=True).clamp_min(1e-12)).contiguous()
    labels = torch.full((M,), -1, dtype=torch.int32, device=x.device)
    n_iter, counts = 0, None
    while n_iter < max_iter:
        changed, counts = _native.ops().kmeans_step(x, centers, labels)
        n_iter += 1
        if int(changed.item()) == 0:
            break
    out = centers.cpu().numpy()
    if return_info:
        return out, {"labels": labels.cpu().numpy(), "counts": counts.cpu().numpy(), "n_iter": n_iter}
    return out
