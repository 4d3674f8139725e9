"""SuperGlue on the GPU (``mlg_superglue``, include/mlgate.h): the matcher the reference's
``SuperGlue`` class configures (scripts/semantic_gating/geometric_verification.py:353-421:
magicleap SuperPoint nms_radius 4 / keypoint_threshold 0.005 / max_keypoints 2048 and
SuperGlue weights 'indoor', sinkhorn_iterations 20, match_threshold 0.2) and whose native
branch it leaves unwritten (:419-421).  Semantics: magicleap's models/superglue.py,
restated in oracle/superglue.py; kernels: csrc/superglue.hip.

Host-side weight preparation: eval BatchNorm folded into the preceding Conv1d, the
attention heads made contiguous (magicleap's ``view(b, 64, 4, n)`` puts head h's dim d
on channel d * 4 + h: the q / k / v rows and the merge columns are permuted to
h * 64 + d), the 256 / 512-wide linears packed k-step-major for the LightGlue block
kernels they reuse (mlgate.lightglue.pack_kstep).
"""
import numpy as np
import torch

from . import _native
from .lightglue import pack_kstep
from .weights import SG_KENC, SG_LAYERS, given_or_resolved

SINKHORN_ITERATIONS = 20
MATCH_THRESHOLD = 0.2


def head_major():
    """perm[h * 64 + d] = d * 4 + h (magicleap channel of head h, dim d)."""
    h, d = np.meshgrid(np.arange(4), np.arange(64), indexing="ij")
    return (d * 4 + h).reshape(-1)


def fold_bn1d(w, b, sd, bn, eps=1e-5):
    """Conv1d weight [o, i, 1] / bias [o] (+ eval BatchNorm1d ``bn``) -> ([o, i], [o]) float32."""
    w = np.asarray(w, np.float32)[:, :, 0]
    b = np.asarray(b, np.float32)
    if bn is None:
        return w, b
    g = sd[bn + ".weight"] / np.sqrt(sd[bn + ".running_var"] + np.float32(eps))
    return (w * g[:, None]).astype(np.float32), ((b - sd[bn + ".running_mean"]) * g + sd[bn + ".bias"]).astype(
        np.float32)


def weight_list(sd, device, gemm_dtype=torch.bfloat16):
    """The torch.ops.mlgate.superglue weight list on ``device``; GEMM weights
    in ``gemm_dtype`` (bf16 for the kernels; float32 lets tests check the layout exactly)."""
    dev = torch.device(device)
    bf = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev).to(gemm_dtype)  # noqa: E731
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    n = len(SG_KENC) - 1
    kenc = [fold_bn1d(sd[f"kenc.encoder.{3 * i}.weight"], sd[f"kenc.encoder.{3 * i}.bias"], sd,
                      f"kenc.encoder.{3 * i + 1}" if i < n - 1 else None) for i in range(n)]
    out = [f32(w) for w, _ in kenc[:3]] + [f32(b) for _, b in kenc[:3]]
    out += [bf(kenc[3][0]), f32(kenc[3][1]), bf(kenc[4][0]), f32(kenc[4][1])]
    perm = head_major()
    for i in range(SG_LAYERS):
        p = f"gnn.layers.{i}."
        proj = [fold_bn1d(sd[p + f"attn.proj.{k}.weight"], sd[p + f"attn.proj.{k}.bias"], sd, None) for k in range(3)]
        wm, bm = fold_bn1d(sd[p + "attn.merge.weight"], sd[p + "attn.merge.bias"], sd, None)
        w1, b1 = fold_bn1d(sd[p + "mlp.0.weight"], sd[p + "mlp.0.bias"], sd, p + "mlp.1")
        w2, b2 = fold_bn1d(sd[p + "mlp.3.weight"], sd[p + "mlp.3.bias"], sd, None)
        out += [bf(pack_kstep(np.concatenate([w[perm] for w, _ in proj]))),
                f32(np.concatenate([b[perm] for _, b in proj])),
                bf(pack_kstep(wm[:, perm])), f32(bm), bf(pack_kstep(w1)), f32(b1), bf(pack_kstep(w2)), f32(b2)]
    wf, bfin = fold_bn1d(sd["final_proj.weight"], sd["final_proj.bias"], sd, None)
    return out + [bf(wf), f32(bfin)]


class SuperGlueGPU:
    """Batched SuperGlue over a ragged set of keyframe pairs on the HIP device."""

    def __init__(self, state_dict=None, device="cuda", sinkhorn_iterations=SINKHORN_ITERATIONS,
                 match_threshold=MATCH_THRESHOLD, weights_path=None, seed=0):
        self.device = _native.require_device(device)
        state_dict, self.weights_source = given_or_resolved("superglue", state_dict, weights_path, seed)
        self.iters = int(sinkhorn_iterations)
        self.threshold = float(match_threshold)
        self.bin_score = float(np.asarray(state_dict["bin_score"], np.float32))
        self._w = weight_list(state_dict, self.device)

    def match_device(self, kpts, scores, desc, counts, pair_a, pair_b, width, height):
        """kpts f32 [F, kmax, 2], scores [F, kmax], desc [F, kmax, 256] on the device; counts,
        pair_a, pair_b host ints; (width, height) the image size the keypoints live in.
        Returns device (matches [P, kmax, 2], match scores [P, kmax], num [P])."""
        host = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.int32)))  # noqa: E731
        return _native.ops().superglue(kpts.contiguous(), scores.contiguous(), desc.contiguous(), host(counts),
                                       host(pair_a), host(pair_b), self._w, self.bin_score, int(width), int(height),
                                       self.iters, self.threshold)

    def match(self, feats0, feats1, width, height):
        """Host convenience for one pair of SuperPoint outputs (dicts of numpy arrays with
        keypoints, keypoint_scores, descriptors): returns (matches [S, 2], scores [S])."""
        k = max(len(feats0["keypoints"]), len(feats1["keypoints"]), 1)
        kp = torch.zeros(2, k, 2, dtype=torch.float32)
        sc = torch.zeros(2, k, dtype=torch.float32)
        ds = torch.zeros(2, k, 256, dtype=torch.float32)
        for j, f in enumerate((feats0, feats1)):
            nk = len(f["keypoints"])
            kp[j, :nk] = torch.as_tensor(np.asarray(f["keypoints"], np.float32))
            sc[j, :nk] = torch.as_tensor(np.asarray(f["keypoint_scores"], np.float32))
            ds[j, :nk] = torch.as_tensor(np.asarray(f["descriptors"], np.float32))
        counts = [len(feats0["keypoints"]), len(feats1["keypoints"])]
        m, s, n = self.match_device(kp.to(self.device), sc.to(self.device), ds.to(self.device), counts, [0], [1],
                                    width, height)
        c = int(n[0])
        return m[0, :c].cpu().numpy(), s[0, :c].cpu().numpy()
