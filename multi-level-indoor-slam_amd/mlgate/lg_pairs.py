"""What DeviceGate and StreamingGate share of the SuperPoint + LightGlue verification: the
feature table, the LightGlue chunk loop over ordered pairs and a chunk's batched RANSAC.  What
a gate does with a chunk's result (streams, tallies, stage marks, poses) stays in pipeline.py.
"""
import numpy as np

from . import _native, gate_plan


class FeatureTable:
    """SuperPoint features, extracted once per keyframe and kept in HBM as flat rows (what
    mlgate.distributed.FeatureExchange moves): kp f32 [rows, KP * 2], ds f32 [rows, KP * 256],
    cnt int32 [rows, 1]."""

    def __init__(self, rows, KP, dev):
        import torch
        self.kp = torch.empty(rows, KP * 2, device=dev)
        self.ds = torch.empty(rows, KP * 256, device=dev)
        self.cnt = torch.zeros(rows, 1, dtype=torch.int32, device=dev)

    def fill(self, sp, frames, dst0, sp_batch):
        """SuperPoint (sp.extract_device) of frames [B, ...] into rows [dst0, dst0 + B), in
        batches of sp_batch on the current stream.  Per-frame results do not depend on which
        frames share a batch."""
        for b0 in range(0, int(frames.shape[0]), sp_batch):
            kp, _, ds, _, cnt = sp.extract_device(frames[b0:b0 + sp_batch])
            dst = slice(dst0 + b0, dst0 + b0 + kp.shape[0])
            self.kp[dst].copy_(kp.flatten(1))
            self.ds[dst].copy_(ds.flatten(1))
            self.cnt[dst, 0].copy_(cnt)


def oriented_matches(lg, kp_all, ds_all, counts, pa, pb, N, chunk, lg_tail=0, dedup=True, row_of=None):
    """LightGlue over the ordered pairs (pa, pb) (host int arrays of keyframes below N), chunk
    by chunk on the current stream.  Yields per chunk (sel, m, n): the positions in (pa, pb) it
    decides and their matches m [P, KP, 2] / n [P] on the device, in each pair's own orientation.
    kp_all [F, KP, 2] / ds_all [F, KP, 256]: the feature views, counts: their keypoint counts on
    the host, row_of: keyframes -> their rows (None: a keyframe is its row).  chunk: unordered
    pairs per LightGlue call, or a function of how many there are that returns it; lg_tail:
    gate_plan.chunk_starts' tail cut; dedup=False: LightGlue on every ordered pair."""
    import torch
    dev = kp_all.device
    # LightGlue once per UNORDERED pair: it is symmetric in its two images (shared
    # weights; self / cross blocks, dual-softmax assignment, early stopping and pruning
    # treat both alike), so (b, a) is (a, b) with the image roles exchanged and the
    # matches re-sorted by the new image0 index (mlg_lg_orient_matches).  Every ORDERED
    # pair still gets its own RANSAC on its own match order and its own decision, as
    # verify_with_semantics gives each (query, match) (geometric_verification.py:688-744).
    ua, ub, inv, swap_all, order = gate_plan.unordered_plan(pa, pb, N, dedup)
    if callable(chunk):
        chunk = chunk(len(ua))
    starts, bounds = gate_plan.chunk_starts(len(ua), chunk, lg_tail, inv[order])
    if row_of is not None:
        ua, ub = row_of(ua), row_of(ub)  # LightGlue indexes the feature tables
    for ci in range(len(starts) - 1):
        c0, c1 = starts[ci], starts[ci + 1]
        mu, su, nu, _ = lg.match_device(kp_all, ds_all, counts, ua[c0:c1], ub[c0:c1])
        sel = order[bounds[ci]:bounds[ci + 1]]  # the ordered pairs of these unordered ones
        if dedup:
            rows = torch.from_numpy((inv[sel] - c0).astype(np.int32)).to(dev)
            sw = torch.from_numpy(swap_all[sel]).to(dev)
            m, _, n = _native.ops().lg_orient(mu, su, nu, rows, sw)
        else:
            m, n = mu, nu
        yield sel, m, n


def ransac_pairs(K, kp_all, m, n, la, lb):
    """geometry.epipolar_ransac_device's whole result (model, mask, inliers, pose, status) of
    one batched RANSAC (+ recoverPose when K is given) over the matched keypoints of P pairs:
    matches m [P, KP, 2] with counts n [P] between rows la / lb (host int arrays) of the
    feature view kp_all.  The flat match arrays are laid out on the device without a host
    sync (no nonzero): pair p's matches go to [offs[p], offs[p] + n[p]) of a buffer of P * KP
    rows (RANSAC reads each pair's own range only), the padding of the match lists to one
    dummy row past the end."""
    import torch
    from . import geometry
    dev, KP, P = kp_all.device, kp_all.shape[1], len(la)
    sidx = torch.arange(KP, device=dev)
    lv = sidx[None, :] < n[:, None]
    la = torch.from_numpy(la).to(dev).long()
    lb = torch.from_numpy(lb).to(dev).long()
    offs = torch.zeros(P + 1, dtype=torch.int32, device=dev)
    offs[1:] = torch.cumsum(n, 0)
    dest = torch.where(lv, offs[:-1, None].long() + sidx[None, :], P * KP).view(-1)
    m0 = torch.where(lv, m[:, :, 0].long(), 0)
    m1 = torch.where(lv, m[:, :, 1].long(), 0)
    k1 = kp_all.new_zeros(P * KP + 1, 2)
    k2 = kp_all.new_zeros(P * KP + 1, 2)
    k1.index_copy_(0, dest, kp_all[la[:, None], m0].view(-1, 2))
    k2.index_copy_(0, dest, kp_all[lb[:, None], m1].view(-1, 2))
    return geometry.epipolar_ransac_device(k1[:P * KP], k2[:P * KP], offs, K, 0, 3.0)
