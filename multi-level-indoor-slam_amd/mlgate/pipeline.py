"""The full semantic loop-closure gate (BASELINE configs[3]).

No reference module chains the gate's stages; SURVEY.md §3.5 defines the harness from
the reference's public APIs, and this module is that harness:

  1. floor labels  IMUFloorDetector.detect_elevator_events / assign_floor_labels
                   (floor_detector.py:63-156), or labels given per keyframe;
  2. descriptors   SemanticPlaceRecognition('cricavpr').add_image per keyframe
                   (place_recognition.py:843-849; here one batched add_images);
  3. retrieval     find_loop_closures(enable_floor_gating, k) (:851-911);
  3a. sequence     (opt-in, seq_radius) the sequence-consistency check of each valid match
                   over the keyframes around it (mlg_seq_gate, include/mlgate.h), before 3b:
                   the matches it rejects reach neither the re-ranking nor the verifier;
  3b. re-ranking   (opt-in, rerank_top_k) CricaVPR.rerank_candidates (:714-757) over each
                   query's valid matches: the first rerank_top_k go on to the verifier;
  4. verification  SemanticGeometricVerifier.verify_with_semantics on every retrieved
                   match with is_valid (geometric_verification.py:688-734; batched);
  5. gate          SemanticLoopClosureGate(floor_labels).gate_candidates on the
                   geometrically valid pairs (loop_closure_gate.py:105-126).

The false-loop-closure rejection count is the sum of four terms:
retrieval matches with PlaceMatch.is_valid False (place_recognition.py:896-899),
verifier skips on a floor mismatch (geometric_verification.py:709-710), verifier
invalid results (:729-732) and the gate's rejected_cross_floor (loop_closure_gate.py:
91-98).

Two front ends run the same kernels:
  * ``FullSemanticGate`` composes the drop-in classes (PlaceMatch / MatchResult /
    LoopClosureCandidate objects, the reference's stats dicts);
  * ``DeviceGate`` is the same chain on device arrays, frame-sharded over ranks (one
    process per GPU, RCCL all-gathers; bench.py's step).  Its decisions and counts are
    those of FullSemanticGate (tests/test_pipeline_gpu.py).
``StreamingGate`` is DeviceGate for keyframes that arrive one batch at a time: after any
sequence of appends its lists, per-pair results and counts are DeviceGate.step()'s on the
keyframes seen so far (tests/test_streaming_gate_gpu.py); the two share mlgate.lg_pairs (feature
table, LightGlue chunk loop, RANSAC call) and gate_plan's floor coding.
"""
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np

from . import _native, gate_plan, lg_pairs, stream_plan

from .floors import IMUFloorDetector
from .gate import LoopClosureCandidate, SemanticLoopClosureGate
from .verify import MatchResult, SemanticGeometricVerifier
from .vpr import PlaceMatch, SemanticPlaceRecognition


@dataclass
class RejectionCount:
    """The four terms of the false-loop-closure rejection count."""
    retrieval_floor_rejected: int = 0   # PlaceMatch.is_valid == False
    skipped_floor_mismatch: int = 0     # SemanticGeometricVerifier skip branch
    verifier_invalid: int = 0           # geometric verification failed
    gate_rejected_cross_floor: int = 0  # SemanticLoopClosureGate rejections

    @property
    def total(self) -> int:
        return (self.retrieval_floor_rejected + self.skipped_floor_mismatch + self.verifier_invalid
                + self.gate_rejected_cross_floor)

    def as_dict(self) -> Dict[str, int]:
        return {'retrieval_floor_rejected': self.retrieval_floor_rejected,
                'skipped_floor_mismatch': self.skipped_floor_mismatch,
                'verifier_invalid': self.verifier_invalid,
                'gate_rejected_cross_floor': self.gate_rejected_cross_floor, 'total': self.total}


@dataclass
class GateReport:
    floor_labels: np.ndarray
    events: list
    matches: List[PlaceMatch]
    verified: List[PlaceMatch]          # matches sent to the verifier, in emission order
    results: List[MatchResult]          # one per verified match
    accepted: List[LoopClosureCandidate]
    rejected: List[LoopClosureCandidate]
    retrieval_stats: Dict
    verifier_stats: Dict
    gate_stats: Dict
    rejections: RejectionCount = field(default_factory=RejectionCount)
    # rerank_top_k: the matches the re-ranking stage did not keep (not a rejection term)
    reranked_out: List[PlaceMatch] = field(default_factory=list)
    # seq_radius: the matches the sequence-consistency check rejected (not a rejection term)
    sequence_rejected: List[PlaceMatch] = field(default_factory=list)


def floor_labels_from_imu(timestamps, imu, start_floor=5, detector_kwargs=None):
    """(labels, events) from an IMU log (t, ax, ay, az) -- floor_detector.py:63-156."""
    det = IMUFloorDetector(**(detector_kwargs or {}))
    t, ax, ay, az = imu[:4]
    events = det.detect_elevator_events(np.asarray(t), np.asarray(ax), np.asarray(ay), np.asarray(az))
    return det.assign_floor_labels(np.asarray(timestamps), start_floor=start_floor), events


class FullSemanticGate:
    """IMU floors -> CricaVPR descriptors -> floor-gated kNN -> semantic geometric
    verification -> floor gate, composed from the drop-in API."""

    def __init__(self, vpr_method: str = 'cricavpr', matcher_type: str = 'lightglue', device: str = 'cuda',
                 similarity_threshold: float = 0.5, min_time_gap: float = 10.0, k: int = 10, min_inliers: int = 20,
                 min_inlier_ratio: float = 0.25, strict_mode: bool = True, retrieval_floor_gating: bool = True,
                 verifier_floor_gating: bool = True, verify_rejected: bool = False, start_floor: int = 5,
                 imu_detector_kwargs: Optional[Dict] = None, backbone: str = 'dinov2_vitb14',
                 rerank_top_k: Optional[int] = None, seq_radius: Optional[int] = None, seq_threshold: float = 0.3,
                 seq_min_terms: int = 2):
        self.vpr_method, self.matcher_type, self.device = vpr_method, matcher_type, device
        # seq_radius: the sequence-consistency check between retrieval and re-ranking, as
        # DeviceGate(seq_radius=...) runs it; None: no such stage
        self.seq_radius, self.seq_threshold, self.seq_min_terms = _seq_args(seq_radius, seq_threshold, seq_min_terms, k)
        # rerank_top_k: CricaVPR.rerank_candidates (place_recognition.py:714-757) between
        # retrieval and verification, as DeviceGate(rerank_top_k=...) runs it; None: no such stage
        self.rerank_top_k = _rerank_arg(
            rerank_top_k, k, vpr_method == 'cricavpr',
            f"rerank_top_k needs CricaVPR's cached local features; the {vpr_method} method caches none")
        # the DINOv2 backbone of the 'cricavpr' / 'anyloc' methods (dinov2_vits14 / b14 / l14)
        self.backbone = backbone
        self.similarity_threshold, self.min_time_gap, self.k = similarity_threshold, min_time_gap, k
        self.min_inliers, self.min_inlier_ratio, self.strict_mode = min_inliers, min_inlier_ratio, strict_mode
        self.retrieval_floor_gating = retrieval_floor_gating
        self.verifier_floor_gating = verifier_floor_gating
        self.verify_rejected = verify_rejected  # also send is_valid == False matches to the verifier
        self.start_floor = start_floor
        self.imu_detector_kwargs = imu_detector_kwargs
        self.spr = None
        self.verifier = None
        self.gate = None

    def run(self, images, timestamps, K: Optional[np.ndarray] = None, floor_labels=None, imu=None) -> GateReport:
        """images: uint8 [N, H, W, C] device tensor or N numpy images; timestamps [N];
        floor labels given, or derived from ``imu`` = (t, ax, ay, az)."""
        import torch
        timestamps = np.asarray(timestamps, np.float64)
        events = []
        if floor_labels is None:
            if imu is None:
                raise ValueError("need floor_labels or an IMU log")
            floor_labels, events = floor_labels_from_imu(timestamps, imu, self.start_floor, self.imu_detector_kwargs)
        floor_labels = np.asarray(floor_labels)
        self.spr = SemanticPlaceRecognition(self.vpr_method, self.device, self.similarity_threshold,
                                            self.min_time_gap)
        if self.backbone != 'dinov2_vitb14':
            from .weights import backbone_config
            if not hasattr(self.spr.vpr, 'backbone_name'):
                raise ValueError(f"backbone = {self.backbone}: the {self.vpr_method} method has no DINOv2 backbone")
            self.spr.vpr.backbone_name = self.backbone
            self.spr.vpr.descriptor_dim = backbone_config(self.backbone)[0]
        if isinstance(images, torch.Tensor):
            frames = images
        else:
            frames = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(im, np.uint8) for im in images])))
        frames = frames.to(torch.device(self.device))
        labels = [int(f) if np.issubdtype(type(f), np.integer) else f for f in floor_labels.tolist()]
        self.spr.add_images(frames, timestamps.tolist(), labels)
        matches = self.spr.find_loop_closures(enable_floor_gating=self.retrieval_floor_gating, k=self.k)
        to_verify = [m for m in matches if m.is_valid or self.verify_rejected]
        sequence_rejected, reranked_out = [], []
        if self.seq_radius is not None:
            to_verify, sequence_rejected = self._sequence(to_verify, len(timestamps))
        if self.rerank_top_k is not None:
            to_verify, reranked_out = self._rerank(to_verify, len(timestamps))
        self.verifier = SemanticGeometricVerifier(self.matcher_type, self.device, self.min_inliers,
                                                  self.min_inlier_ratio, enable_floor_gating=self.verifier_floor_gating)
        pairs = [(m.query_idx, m.match_idx) for m in to_verify]
        results = self.verifier.verify_with_semantics_batch(frames, pairs,
                                                            [(labels[a], labels[b]) for a, b in pairs], K, pairs)
        self.gate = SemanticLoopClosureGate(floor_labels, strict_mode=self.strict_mode)
        accepted, rejected = self.gate.gate_candidates(
            [(m.query_idx, m.match_idx, m.similarity) for m, r in zip(to_verify, results) if r.is_valid])
        vstats = self.verifier.get_statistics()
        gstats = self.gate.get_stats()
        counts = RejectionCount(retrieval_floor_rejected=sum(1 for m in matches if not m.is_valid),
                                skipped_floor_mismatch=vstats['skipped_floor_mismatch'],
                                verifier_invalid=vstats['invalid'],
                                gate_rejected_cross_floor=gstats['rejected_cross_floor'])
        return GateReport(floor_labels=floor_labels, events=events, matches=matches, verified=to_verify,
                          results=results, accepted=accepted, rejected=rejected,
                          retrieval_stats=self.spr.get_statistics(matches), verifier_stats=vstats,
                          gate_stats=gstats, rejections=counts, reranked_out=reranked_out,
                          sequence_rejected=sequence_rejected)

    @staticmethod
    def _rows(to_verify, n):
        """The matches bound for the verifier as knn_gate-shaped host lists: (rows, idx, sim,
        count), each query's matches in emission order."""
        rows = {}
        for m in to_verify:
            rows.setdefault(m.query_idx, []).append(m)
        k = max([len(r) for r in rows.values()] + [1])
        idx, sim = np.zeros((n, k), np.int32), np.zeros((n, k), np.float32)
        count = np.zeros(n, np.int32)
        for q, r in rows.items():
            idx[q, :len(r)] = [m.match_idx for m in r]
            sim[q, :len(r)] = [m.similarity for m in r]
            count[q] = len(r)
        return rows, idx, sim, count

    def _sequence(self, to_verify, n):
        """(kept, rejected) of the matches bound for the verifier, through mlg_seq_gate over
        the descriptors, timestamps and floor codes find_loop_closures used; order unchanged."""
        import torch
        from . import retrieval
        if not to_verify:
            return [], []
        rows, idx, sim, count = self._rows(to_verify, n)
        descs = self.spr.vpr.descriptors
        X, dev = self.spr.vpr._device_matrix()
        codes, has = gate_plan.floor_codes([d.floor_label for d in descs])
        keep = retrieval.sequence_gate(
            X, torch.tensor([float(d.timestamp) for d in descs], dtype=torch.float64, device=dev),
            torch.from_numpy(codes).to(dev), torch.from_numpy(has).to(dev), torch.from_numpy(idx).to(dev),
            torch.from_numpy(sim).to(dev), None, torch.from_numpy(count).to(dev), self.seq_radius,
            self.seq_threshold, self.min_time_gap, self.seq_min_terms)[3].cpu().numpy()
        kept, rejected = [], []
        seen = {}
        for m in to_verify:  # a query's matches are in its row in the order they appear here
            s = seen[m.query_idx] = seen.get(m.query_idx, -1) + 1
            (kept if keep[m.query_idx, s] else rejected).append(m)
        return kept, rejected

    def _rerank(self, to_verify, n):
        """(kept, dropped) of the matches bound for the verifier: each query's matches, in
        emission order, through mlg_rerank_gate over the cached local features; the kept ones
        row-major by query and in re-ranked order within a row, similarities unchanged."""
        import torch
        from . import retrieval
        vpr = self.spr.vpr
        rows, idx, sim, count = self._rows(to_verify, n)
        k = idx.shape[1]
        cache = vpr._feature_cache if vpr.use_reranking else {}
        cached = np.array([f in cache for f in range(n)], np.uint8)
        some = next(iter(cache.values())) if cache else None
        if some is None:  # nothing cached: every row keeps its first top_k
            bank = torch.zeros(n, 1, 4, device=torch.device(self.device))
        else:
            some = vpr._to_device_feats(some)
            bank = torch.zeros((n,) + tuple(some.shape), device=some.device)
            for f, v in cache.items():
                bank[f].copy_(vpr._to_device_feats(v))
        dev = bank.device
        r_idx, _, _, _, r_count = retrieval.rerank_gate(
            bank, torch.from_numpy(idx).to(dev), torch.from_numpy(sim).to(dev), None, torch.from_numpy(count).to(dev),
            min(self.rerank_top_k, k), cached=torch.from_numpy(cached).to(dev))
        r_idx, r_count = r_idx.cpu().numpy(), r_count.cpu().numpy()
        kept = []
        for q in sorted(rows):
            by_idx = {m.match_idx: m for m in rows[q]}
            kept += [by_idx[int(j)] for j in r_idx[q, :r_count[q]]]
        keep_ids = {id(m) for m in kept}
        return kept, [m for m in to_verify if id(m) not in keep_ids]


def _seq_args(seq_radius, seq_threshold, seq_min_terms, k):
    """(radius or None, threshold, min_terms) of both gates' seq_* arguments, refused before
    anything is built: the kernel takes a radius in [1, 7] and a lane per slot (k <= 64)."""
    if seq_radius is None:
        return None, float(seq_threshold), int(seq_min_terms)
    if not 1 <= int(seq_radius) <= 7:
        raise ValueError(f"seq_radius must be in [1, 7] (got {seq_radius})")
    if int(seq_min_terms) < 1:
        raise ValueError(f"seq_min_terms must be >= 1 (got {seq_min_terms})")
    if int(k) > 64:
        raise ValueError(f"seq_radius takes k <= 64 (got k = {k})")
    return int(seq_radius), float(seq_threshold), int(seq_min_terms)


def _rerank_arg(rerank_top_k, k, has_local_features, why_not):
    """rerank_top_k (int or None) of both gates, refused before anything is built: without the
    gate's local features (ValueError(why_not)), below 1, or with more slots than lanes (k > 64)."""
    if rerank_top_k is None:
        return None
    if not has_local_features:
        raise ValueError(why_not)
    if int(rerank_top_k) < 1:
        raise ValueError(f"rerank_top_k must be >= 1 (got {rerank_top_k})")
    if int(k) > 64:
        raise ValueError(f"rerank_top_k takes k <= 64 (got k = {k})")
    return int(rerank_top_k)


def _camera_matrix(torch, K, dev):
    """The camera matrix (3x3 array-like, or None) as the f64 [9] device tensor RANSAC takes."""
    return None if K is None else torch.from_numpy(np.asarray(K, np.float64).reshape(9).copy()).to(dev)


def _vit_engine(vit_state_dict, backbone, dev, vit_batch, vit_precise):
    """The gates' ViT engine; vit_state_dict None: the synthetic weights of seed 0."""
    from .vit import engine_for
    from .weights import synthetic_state_dict
    sd = vit_state_dict if vit_state_dict is not None else synthetic_state_dict(0, backbone)
    # vit_precise: the split-bf16 ViT (MLG_VIT_SPLIT), whose descriptors follow the fp32
    # network closely enough that the kNN ranks near-ties as the fp32 reference does
    return engine_for(sd, backbone, device=dev, max_batch=vit_batch, precise=vit_precise)


def decide_pairs(n, inl, ta, tb, f_num, limit, min_inliers, min_inlier_ratio, n_valid_t, gate_rej_t):
    """The verifier's decision rule (geometric_verification.py:602-620) and the floor gate
    (loop_closure_gate.py:91-98) for a chunk of pairs, on tensors of any one device: match
    counts n and inlier counts inl [P], keyframe indices ta / tb [P] (int64) into the numeric
    floor labels f_num.  Returns ok [P] and adds the geometrically valid pairs to n_valid_t,
    those of them the floor gate rejects to gate_rej_t (0-d int64), with no host sync.
    Deviation, by design: a None label is NaN in f_num and never rejects, where the
    reference's host gate computes abs(None - None) and raises TypeError
    (loop_closure_gate.py:89; the drop-in SemanticLoopClosureGate keeps that TypeError,
    tests/test_api_cpu.py::test_gate_none_labels_raise_nan_labels_accept)."""
    ratio = inl.double() / n.clamp(min=1).double()
    ok = (n >= 5) & (inl >= min_inliers) & (ratio >= min_inlier_ratio)
    n_valid_t += ok.sum()
    gate_rej_t += (ok & ((f_num[ta] - f_num[tb]).abs() > limit)).sum()
    return ok


class DeviceGate:
    """The same chain on device arrays for a frame-sharded sequence: rank r of W owns
    keyframes [r N / W, (r + 1) N / W) -- its frames, ViT forwards and SuperPoint
    features -- and the query rows of the same range.  Exchange steps (RCCL over
    xGMI; gloo through host copies): the [N, 768] descriptor all-gather before retrieval,
    an 8-B-per-pair all-gather that re-balances the gate-accepted pairs across ranks
    (mlgate.distributed.balanced_pairs), and the SuperPoint features of exactly the
    keyframes each rank's pair slice touches (mlgate.distributed.FeatureExchange).

    One ``step()`` gates the whole sequence once and returns per-rank counts; the
    caller all-reduces them (bench.py)."""

    def __init__(self, frames, timestamps, floor_labels, world=1, rank=0, device='cuda', k=10,
                 similarity_threshold=0.5, min_time_gap=10.0, strict_mode=True, retrieval_floor_gating=True,
                 verifier_floor_gating=True, verify=True, K=None, min_inliers=20, min_inlier_ratio=0.25,
                 vit_batch=123, sp_batch=64, lg_chunk=1024, max_keypoints=2048, vit_state_dict=None, record=False,
                 vit_precise=True, matcher='lightglue', loftr_chunk=256, max_pairs=None, lg_tail=0,
                 local_features=True, backbone='dinov2_vitb14', rerank_top_k=None, overlap=True, lg_dedup=True,
                 seq_radius=None, seq_threshold=0.3, seq_min_terms=2):
        # seq_radius: the sequence-consistency check (mlg_seq_gate, include/mlgate.h) of the
        # valid entries of each query row, after retrieval and before re-ranking: a match whose
        # neighbouring keyframes do not match in either travel direction goes no further.
        # None: the stage does not exist.  With several ranks nothing new is exchanged: every
        # rank holds the gathered [N, D] descriptors and judges its own rows.
        self.seq_radius, self.seq_threshold, self.seq_min_terms = _seq_args(seq_radius, seq_threshold, seq_min_terms, k)
        self.last_sequence = None
        self.rerank_top_k = _rerank_arg(rerank_top_k, k, local_features,
                                        "rerank_top_k needs the local features: local_features=True")
        import torch
        from . import distributed as mdist
        from .lightglue import LightGlueGPU
        from .superpoint import SuperPointGPU
        from .weights import backbone_config
        self.torch, self.mdist = torch, mdist
        # the DINOv2 backbone: its width sizes the gather, descriptor and local-feature buffers
        self.backbone = backbone
        EMBED = backbone_config(backbone)[0]
        self.dev = torch.device(device)
        self.world, self.rank = world, rank
        N = self.N = len(timestamps)
        self.lo, self.hi = mdist.shard(N, world, rank)
        self.n_local = self.hi - self.lo
        if frames.shape[0] != self.n_local:
            raise ValueError(f"rank {rank} owns {self.n_local} keyframes, got {frames.shape[0]} frames")
        self.frames = frames
        self.k, self.thr, self.gap = int(k), float(similarity_threshold), float(min_time_gap)
        self.limit = 0 if strict_mode else 1
        self.retrieval_floor_gating, self.verifier_floor_gating = retrieval_floor_gating, verifier_floor_gating
        self.min_inliers, self.min_inlier_ratio = min_inliers, min_inlier_ratio
        # lg_chunk: pairs per LightGlue call, or 'auto' (sized from the free HBM when the pairs
        # are known: _lg_chunk_for)
        self.sp_batch, self.lg_chunk, self.kp = sp_batch, lg_chunk, max_keypoints
        self.lg_tail = int(lg_tail)
        self.t_all = torch.as_tensor(np.asarray(timestamps, np.float64), device=self.dev)
        self.labels = np.asarray(floor_labels)
        # equality codes for the retrieval floor check and the verifier skip (Python ==
        # semantics: 1 == 1.0, NaN != NaN, None = no label), the numeric labels for the
        # gate's |floor_i - floor_j| > limit (loop_closure_gate.py:91-98; NaN never rejects)
        lab = gate_plan.label_list(self.labels)
        self.h_codes, self.h_has = gate_plan.floor_codes(lab)  # int64, uint8
        self.f_all = torch.as_tensor(self.h_codes, device=self.dev)
        self.hf_all = torch.as_tensor(self.h_has, device=self.dev)
        self.f_num = torch.as_tensor(gate_plan.numeric_labels(lab), device=self.dev)
        self.eng = _vit_engine(vit_state_dict, backbone, self.dev, vit_batch, vit_precise)
        self.gather = mdist.RowGather(N, EMBED, world, self.dev)
        self.desc_loc = (self.gather.out[self.lo:self.hi] if world == 1
                         else torch.empty(self.n_local, EMBED, device=self.dev))
        # CricaVPR's per-keyframe local features (place_recognition.py:645-667, the input of
        # rerank_candidates), written by the same ViT forward: [N, 528, 768] f32 at ViT-B, 1.6 MB per
        # keyframe.  local_features=False leaves them unmaterialised (the gate reads them only
        # with rerank_top_k): the N = 19,163 sequence then fits one GPU with its LightGlue workspace
        self.local_feats = (torch.empty(self.n_local, self.eng.n_local, EMBED, dtype=torch.float32, device=self.dev)
                            if local_features else None)
        self.totals = torch.zeros(2, dtype=torch.int64, device=self.dev)
        # rerank_top_k: CricaVPR.rerank_candidates (place_recognition.py:714-757) between
        # retrieval and verification -- the valid entries of each query row re-ranked by
        # 0.5 global + 0.5 local cross-correlation, the first rerank_top_k handed to the
        # verifier (mlg_rerank_gate).  None: the stage does not exist.  With several ranks the
        # bank of local features is all-gathered: every rank then holds all N keyframes'
        # [528, EMBED] f32 features (1.6 MB per keyframe at ViT-B)
        if self.rerank_top_k is not None:
            self.feat_gather = (mdist.RowGather(N, self.eng.n_local * EMBED, world, self.dev) if world > 1
                                else None)
        self.last_rerank = None
        self.verify = verify
        # matcher: 'lightglue' (SuperPoint + LightGlue, the reference default) or 'loftr'
        # (GeometricVerifier('loftr'), geometric_verification.py:424-526; BASELINE configs[4])
        if matcher not in ('lightglue', 'loftr'):
            raise ValueError(f"Unknown matcher: {matcher}")
        self.matcher = matcher
        self.loftr_chunk = int(loftr_chunk)
        self.max_pairs = max_pairs  # verify only the first max_pairs pairs of the global list (bench sub-runs)
        if verify:
            self.fx = mdist.FeatureExchange(N, world, rank) if world > 1 else None
            self.K = _camera_matrix(torch, K, self.dev)
        if verify and matcher == 'loftr':
            from .loftr import LoFTRGPU
            self.lf = LoFTRGPU(device=self.dev, feature_batch=16)
        elif verify:
            self.sp = SuperPointGPU(device=self.dev, max_num_keypoints=max_keypoints)
            self.lg = LightGlueGPU(device=self.dev)
            # this rank's keyframes' features; with world > 1 each rank then receives the
            # features of exactly the keyframes its verification slice touches
            self.feats = lg_pairs.FeatureTable(self.n_local, max_keypoints, self.dev)
            self.kp_loc, self.ds_loc, self.cnt_loc = self.feats.kp, self.feats.ds, self.feats.cnt
        # overlap=True: the step on a high-priority stream, SuperPoint on a side stream under
        # the ViT and the kNN, each LightGlue chunk's RANSAC on a side stream under the next
        # chunk (step, _step, _verify_lightglue).  overlap=False: everything on the caller's
        # current stream at normal priority, in program order -- the same results (tests/
        # test_pipeline_gpu.py::test_stream_overlap_changes_nothing) and serial stage times.
        # lg_dedup=False: LightGlue on every ordered pair, not once per unordered pair.
        self.overlap, self.lg_dedup = bool(overlap), bool(lg_dedup)
        self._hi = self._sp_stream = self._side = None  # made by the first overlapped step
        # record=True: step() keeps every verified ordered pair's (a, b, matches, inliers,
        # is_valid) in self.last_pair_results (host arrays in verification order)
        self.record = record
        # time_verify=True: _verify_loftr brackets its work with device syncs and leaves the
        # wall time in last_verify_s (bench.py's LoFTR sub-run); off, the gate never syncs for it
        self.time_verify = False
        self.last_verify_s = None
        self.last_pair_results = None
        self.last_retrieval = None
        self.last_pairs = None

    def step(self):
        """Gate the sequence once.  Returns this rank's counts (dict of ints): matches,
        the four rejection terms, pairs verified, pairs geometrically valid, accepted.
        The step's own work runs on a high-priority stream, so the hardware dispatches its
        workgroups ahead of the side streams' (RANSAC, SuperPoint): they fill the gaps and
        kernel tails instead of taking CUs from the LightGlue kernels (same-box A/B,
        profiles/r06p_ab_main_priority.txt: attention -2 % per launch, step time equal).
        overlap=False: everything on the caller's stream, at normal priority."""
        if not self.overlap:
            return self._step()
        torch = self.torch
        if self._hi is None:
            self._hi = torch.cuda.Stream(device=self.dev, priority=-1)
            if self.verify and self.matcher == 'lightglue':  # SuperPoint's and RANSAC's side streams
                self._sp_stream, self._side = torch.cuda.Stream(device=self.dev), torch.cuda.Stream(device=self.dev)
        cur = torch.cuda.current_stream(self.dev)
        self._hi.wait_stream(cur)
        with torch.cuda.stream(self._hi):
            out = self._step()
        cur.wait_stream(self._hi)
        return out

    def _step(self):
        torch = self.torch
        from . import retrieval
        lightglue = self.verify and self.matcher == 'lightglue'
        # SuperPoint of every local keyframe on its side stream (normal priority) while the
        # ViT and the kNN run on this one (high priority): it fills the ViT kernels' tails and
        # the CUs its LayerNorm / attention launches leave free (same-box ABAB, profiles/
        # r06u_ab_sp_under_vit.txt: -0.4 % step time, counts identical).  The LightGlue stage
        # waits on its event.  overlap=False: SuperPoint after them on this stream.
        sp_ev = self._extract_side() if lightglue and self.overlap else None
        self.eng.forward_into(self.frames, self.desc_loc, self.local_feats)
        if self.world > 1:
            self.gather(self.desc_loc)  # RCCL all-gather of the descriptors over xGMI
        self.totals.zero_()
        idx, sim, valid, count = retrieval.knn_gate(self.gather.out, self.t_all, self.f_all, self.hf_all, self.gap,
                                                    self.thr, self.k, self.retrieval_floor_gating, q0=self.lo,
                                                    Q=self.n_local, totals=self.totals)
        # the retrieval lists come to the host once (Q x k entries): the pair list that
        # drives the verifier's chunks is built there, with no further device syncs
        rr = sq = ()
        cand = valid  # the entries that go on: the valid ones, then those the sequence check keeps
        if self.seq_radius is not None:
            sq = retrieval.sequence_gate(self.gather.out, self.t_all, self.f_all, self.hf_all, idx, sim, valid, count,
                                         self.seq_radius, self.seq_threshold, self.gap, self.seq_min_terms, q0=self.lo)
            cand = sq[3]
        if self.rerank_top_k is not None:
            bank = self.local_feats
            if self.world > 1:  # every rank's keyframes' local features, in keyframe order
                bank = self.feat_gather(self.local_feats.view(self.n_local, -1)).view(
                    self.N, self.local_feats.shape[1], self.local_feats.shape[2])
            rr = retrieval.rerank_gate(bank, idx, sim, cand, count, min(self.rerank_top_k, idx.shape[1]),
                                       q0=self.lo)
        h_idx, h_valid, h_count, *h_more = (x.cpu().numpy() for x in (idx, valid, count) + tuple(sq) + tuple(rr))
        h_sq, h_rr = h_more[:len(sq)], h_more[len(sq):]
        if self.record:  # this rank's query rows: idx / sim / valid [Q, k], count [Q] (host)
            self.last_retrieval = (h_idx, sim.cpu().numpy(), h_valid, h_count)
        matches, floor_rej, pa_h, pb_h = gate_plan.pairs_from_retrieval(h_idx, h_valid, h_count, self.lo)
        out = {"matches": matches, "retrieval_floor_rejected": floor_rej, "skipped_floor_mismatch": 0,
               "verifier_invalid": 0, "gate_rejected_cross_floor": 0, "pairs_verified": 0, "verified_valid": 0,
               "accepted": 0}
        if h_sq:
            # the sequence check on: the entries it kept, in emission order.  sequence_rejected
            # is not a rejection term either
            if self.record:  # s_score / s_dir / s_terms / keep [Q, k] (host)
                self.last_sequence = tuple(h_sq)
            out["sequence_candidates"] = len(pa_h)
            pa_h, pb_h = gate_plan.pairs_from_sequence(h_idx, h_sq[3], self.lo)
            out["sequence_rejected"] = out["sequence_candidates"] - len(pa_h)
        if h_rr:
            # re-ranking on: the kept entries instead, in re-ranked order within a row.
            # reranked_out is not a rejection term (RejectionCount keeps its four)
            if self.record:  # r_idx / r_sim / r_cross / r_score [Q, top_k], r_count [Q] (host)
                self.last_rerank = tuple(h_rr)
            out["rerank_candidates"] = len(pa_h)
            pa_h, pb_h = gate_plan.pairs_from_rerank(h_rr[0], h_rr[4], self.lo)
            out["reranked_out"] = out["rerank_candidates"] - len(pa_h)
        if self.record:  # the ordered pairs bound for the verifier, before its floor skip (host int32)
            self.last_pairs = (pa_h, pb_h)
        if not self.verify:
            return out
        # SuperPoint once per keyframe (the reference re-extracts per pair), cached in HBM
        if sp_ev is not None:
            torch.cuda.current_stream(self.dev).wait_event(sp_ev)
        elif lightglue:
            self.feats.fill(self.sp, self.frames, 0, self.sp_batch)
        if self.verifier_floor_gating:  # the verifier's skip rule on floors
            same = gate_plan.same_floor(pa_h, pb_h, self.h_codes, self.h_has)
            out["skipped_floor_mismatch"] = int((~same).sum())
            pa_h, pb_h = pa_h[same], pb_h[same]
        pa_t, pb_t = torch.from_numpy(pa_h).to(self.dev), torch.from_numpy(pb_h).to(self.dev)
        if self.matcher == 'loftr':
            return self._verify_loftr(pa_t, pb_t, out)
        # pair-level load balance across ranks: the pairs are re-balanced first (the union
        # of the slices is the global pair list), then FeatureExchange delivers each rank
        # exactly the SuperPoint features its own slice touches
        if self.world > 1:
            pa_t, pb_t = self.mdist.balanced_pairs(pa_t, pb_t, self.world, self.rank, group_reverse=self.lg_dedup)
            pa, pb = pa_t.cpu().numpy(), pb_t.cpu().numpy()
        else:
            pa, pb = pa_h, pb_h
        return self._verify_lightglue(pa, pb, out)

    def _verify_lightglue(self, pa, pb, out):
        """SuperPoint features (local table or need-driven exchange) -> LightGlue (once per
        unordered pair with lg_dedup) -> RANSAC + decision + floor gate per ordered pair, for
        this rank's slice (pa, pb) of the pair list (host int32 arrays); fills `out`."""
        torch = self.torch
        self.last_pairs = (pa, pb)
        # features of the keyframes the pairs touch: the local table (world 1), or the
        # need-driven exchange (row k of the compact tables = keyframe need[k])
        if self.world > 1:
            need = np.unique(np.concatenate([pa, pb]).astype(np.int64))
            kp_t, ds_t, cnt_t = self.fx(need, [self.kp_loc, self.ds_loc, self.cnt_loc])
            nf = len(need)
            local = lambda x: np.searchsorted(need, x).astype(np.int32)  # noqa: E731
            out["features_exchanged_bytes"] = self.fx.last_bytes
        else:
            kp_t, ds_t, cnt_t, nf = self.kp_loc, self.ds_loc, self.cnt_loc, self.N
            local = lambda x: np.asarray(x, np.int32)  # noqa: E731
        kp_all = kp_t.view(nf, self.kp, 2)
        ds_all = ds_t.view(nf, self.kp, 256)
        counts = cnt_t.view(-1).cpu().numpy()

        def chunk_for(n_unordered):  # the pairs LightGlue runs on are known inside lg_pairs
            out["pairs_matched_lightglue"] = n_unordered
            self.last_lg_chunk = self._lg_chunk_for(n_unordered)
            return self.last_lg_chunk
        # RANSAC of chunk c runs on a side stream while LightGlue matches chunk c + 1 on
        # this one (mlg_lightglue waits on its stream once per layer; the side stream
        # fills those gaps and the CUs the small RANSAC / assignment grids leave idle).
        # overlap=False: the side stream is this one
        main = torch.cuda.current_stream(self.dev)
        side = self._side if self.overlap else main
        n_valid_t, gate_rej_t, rec = self._tallies()
        for sel, m, n in lg_pairs.oriented_matches(self.lg, kp_all, ds_all, counts, pa, pb, self.N, chunk_for,
                                                   self.lg_tail, self.lg_dedup, local):
            ca, cb = pa[sel], pb[sel]
            ready = torch.cuda.Event()
            ready.record(main)
            with torch.cuda.stream(side):
                side.wait_event(ready)
                m.record_stream(side)
                n.record_stream(side)
                # (every host -> device copy before the RANSAC launch: a copy waits for its stream)
                ta = torch.from_numpy(ca).to(self.dev).long()  # global keyframe indices
                tb = torch.from_numpy(cb).to(self.dev).long()
                inl = lg_pairs.ransac_pairs(self.K, kp_all, m, n, local(ca), local(cb))[2]
                ok = decide_pairs(n, inl, ta, tb, self.f_num, self.limit, self.min_inliers, self.min_inlier_ratio,
                                  n_valid_t, gate_rej_t)
                if rec is not None:
                    rec.append((sel, n, inl, ok))
        main.wait_stream(side)
        return self._finish(out, pa, pb, n_valid_t, gate_rej_t, rec)

    def _tallies(self):
        """(n_valid_t, gate_rej_t, rec): the two device tallies decide_pairs adds to and,
        with record, the list of the chunks' (sel, n, inl, ok)."""
        z = lambda: self.torch.zeros((), dtype=self.torch.int64, device=self.dev)  # noqa: E731
        return z(), z(), [] if self.record else None

    def _finish(self, out, pa, pb, n_valid_t, gate_rej_t, rec):
        """The verification's one device sync, then last_pair_results (record) and the counts."""
        n_valid, gate_rej = int(n_valid_t), int(gate_rej_t)
        if rec is not None:
            self.last_pair_results = gate_plan.pair_records(
                pa, pb, [(sel,) + tuple(x.cpu().numpy() for x in dev) for sel, *dev in rec])
        out["pairs_verified"] = len(pa)
        out["verified_valid"] = n_valid
        out["verifier_invalid"] = len(pa) - n_valid
        out["gate_rejected_cross_floor"] = gate_rej
        out["accepted"] = n_valid - gate_rej
        return out

    # HBM per LightGlue pair beside its mlg_lightglue workspace: the pair's RANSAC
    # workspace at 1000 hypotheses (models, scores, subsets, points: ~0.9 MB), its flat
    # match coordinates and oriented matches
    _RANSAC_PAIR_BYTES = 1 << 20

    def _lg_chunk_for(self, n_pairs):
        """Pairs per LightGlue call: self.lg_chunk, or with 'auto' the largest multiple of 256
        (<= 5120, bench.py's measured optimum) whose LightGlue + RANSAC workspaces fit in the
        HBM free now (the caching allocator's reusable blocks included), keeping 6 % of the
        device and 4 GiB in reserve."""
        if self.lg_chunk != 'auto':
            return int(self.lg_chunk)
        torch = self.torch
        free, total = torch.cuda.mem_get_info(self.dev)
        free += torch.cuda.memory_reserved(self.dev) - torch.cuda.memory_allocated(self.dev)
        avail = free - 0.06 * total - (4 << 30)
        per = _native.lightglue_workspace_bytes(1024, self.kp) / 1024 + self._RANSAC_PAIR_BYTES
        return gate_plan.auto_chunk(avail, per, n_pairs)

    def _extract_side(self):
        """SuperPoint of every local keyframe into the feature table on the SuperPoint side
        stream, after everything already queued on the current stream; returns the event the
        consumers of the table wait on."""
        torch = self.torch
        main = torch.cuda.current_stream(self.dev)
        sps = self._sp_stream
        sps.wait_stream(main)
        with torch.cuda.stream(sps):
            self.feats.fill(self.sp, self.frames, 0, self.sp_batch)
        done = torch.cuda.Event()
        done.record(sps)
        return done

    def _verify_loftr(self, pa_t, pb_t, out):
        """verify_with_semantics with GeometricVerifier('loftr') on this rank's slice of the
        pairs (geometric_verification.py:469-526 matches, :104-153 RANSAC, :602-620 rule).
        LoFTR is not symmetric in its images (the fine stage refines in image 1), so every
        ordered pair is matched.  Each rank receives the raw frames its slice touches
        (0.9 MB per keyframe; FeatureExchange over uint8 rows) and runs the backbone on
        them: cheaper to move than the 44 MB of coarse + fine features per keyframe.  Pairs
        go in chunks of loftr_chunk, ordered by (query, match); the backbone features of a
        chunk's keyframes are kept across chunks in a buffer of 2 x 2 x loftr_chunk rows
        and recomputed only for keyframes not already held."""
        torch = self.torch
        from . import geometry
        if self.time_verify:
            torch.cuda.synchronize(self.dev)
        t_start = time.perf_counter()
        if self.max_pairs is not None:
            pa_t, pb_t = self._first_pairs(pa_t, pb_t, self.max_pairs)
        pa_t, pb_t = self.mdist.balanced_pairs(pa_t, pb_t, self.world, self.rank)
        pa, pb = pa_t.cpu().numpy().astype(np.int64), pb_t.cpu().numpy().astype(np.int64)
        self.last_pairs = (pa, pb)
        need = np.unique(np.concatenate([pa, pb])) if len(pa) else np.zeros(0, np.int64)
        if self.world > 1:
            fl = self.frames.reshape(self.n_local, -1)
            frames = self.fx(need, [fl])[0].view((len(need),) + tuple(self.frames.shape[1:]))
            out["features_exchanged_bytes"] = self.fx.last_bytes
            row_of = {int(f): i for i, f in enumerate(need)}
        else:
            frames = self.frames
            row_of = None
        H, W = int(frames.shape[1]) // 8 * 8, int(frames.shape[2]) // 8 * 8
        order = np.lexsort((pb, pa))
        C = self.loftr_chunk
        cap = 4 * C
        cache = gate_plan.SlotCache(cap)
        coarse = fine = None
        n_valid_t, gate_rej_t, rec = self._tallies()
        for c0 in range(0, len(order), C):
            sel = order[c0:c0 + C]
            ca, cb = pa[sel], pb[sel]
            todo, slots = cache.assign(np.unique(np.concatenate([ca, cb])))
            if todo:
                rows = [f if row_of is None else row_of[f] for f in todo]
                if row_of is None:
                    rows = [f - self.lo for f in rows]
                cf_, ff_ = self.lf.features(frames[torch.as_tensor(rows, device=self.dev)].contiguous())
                if coarse is None:
                    coarse = torch.empty((cap,) + tuple(cf_.shape[1:]), dtype=cf_.dtype, device=self.dev)
                    fine = torch.empty((cap,) + tuple(ff_.shape[1:]), dtype=ff_.dtype, device=self.dev)
                st = torch.as_tensor(slots, device=self.dev)
                coarse.index_copy_(0, st, cf_)
                fine.index_copy_(0, st, ff_)
            n, k0, k1, _ = self.lf.match_device(coarse, fine, H, W, [cache.slot_of[int(a)] for a in ca],
                                                [cache.slot_of[int(b)] for b in cb])
            n = n.to(self.dev).long()
            P = len(sel)
            lv = torch.arange(k0.shape[1], device=self.dev)[None, :] < n[:, None]
            pi, si = torch.nonzero(lv, as_tuple=True)
            offs = torch.zeros(P + 1, dtype=torch.int32, device=self.dev)
            offs[1:] = torch.cumsum(n, 0)
            _, _, inl, _, _ = geometry.epipolar_ransac_device(k0[pi, si].contiguous(), k1[pi, si].contiguous(),
                                                              offs, self.K, 0, 3.0)
            ta = torch.from_numpy(ca).to(self.dev)
            tb = torch.from_numpy(cb).to(self.dev)
            ok = decide_pairs(n, inl, ta, tb, self.f_num, self.limit, self.min_inliers, self.min_inlier_ratio,
                              n_valid_t, gate_rej_t)
            if rec is not None:
                rec.append((sel, n, inl, ok))
        if self.time_verify:
            torch.cuda.synchronize(self.dev)
            self.last_verify_s = time.perf_counter() - t_start  # this rank's LoFTR verification wall time
        out["pairs_matched_loftr"] = len(pa)
        return self._finish(out, pa, pb, n_valid_t, gate_rej_t, rec)

    def _first_pairs(self, pa_t, pb_t, limit):
        """The first `limit` pairs of the global (rank-ordered) pair list, as this rank's part."""
        if self.world == 1:
            return pa_t[:limit], pb_t[:limit]
        torch = self.torch
        n = torch.tensor([pa_t.numel()], dtype=torch.int64, device=self.dev)
        sizes = [torch.zeros_like(n) for _ in range(self.world)]
        self.mdist.all_gather_into(sizes, n)
        before = sum(int(x.item()) for x in sizes[:self.rank])
        take = max(0, min(pa_t.numel(), limit - before))
        return pa_t[:take], pb_t[:take]



class StreamingGate:
    """DeviceGate for keyframes that arrive one batch at a time: ``append`` gates the new
    keyframes against everything seen and updates what the earlier ones close against, paying
    for the new rows only.  After any sequence of appends the state is what
    ``DeviceGate(...).step()`` computes on the keyframes seen so far -- the retrieval lists bit
    for bit (mlg_knn_append, include/mlgate.h), every per-pair match count, inlier count and
    decision, and every count of ``report()``.  One GPU, the LightGlue matcher; the sequence
    check, the re-ranking and the local features are DeviceGate's alone.  The host side is
    mlgate.stream_plan (CPU-tested); the arguments have DeviceGate's names and meaning."""

    def __init__(self, capacity, device='cuda', k=10, similarity_threshold=0.5, min_time_gap=10.0, strict_mode=True,
                 retrieval_floor_gating=True, verifier_floor_gating=True, verify=True, K=None, min_inliers=20,
                 min_inlier_ratio=0.25, vit_batch=123, sp_batch=64, lg_chunk=1024, max_keypoints=2048,
                 vit_state_dict=None, vit_precise=True, backbone='dinov2_vitb14'):
        if int(capacity) < 1:
            raise ValueError(f"capacity must be >= 1 (got {capacity})")
        if not 1 <= int(k) <= 32:  # refused before anything is built
            raise ValueError(f"StreamingGate takes k in [1, 32] (got k = {k})")
        import torch
        from . import retrieval
        from .lightglue import LightGlueGPU
        from .superpoint import SuperPointGPU
        from .weights import backbone_config
        self.torch = torch
        self.dev = torch.device(device)
        self.capacity, self.k = int(capacity), int(k)
        self.embed = backbone_config(backbone)[0]
        self.verify, self.sp_batch, self.lg_chunk, self.kp = bool(verify), int(sp_batch), int(lg_chunk), max_keypoints
        self.knn = retrieval.StreamingKnn(self.capacity, self.embed, self.k, min_time_gap, similarity_threshold,
                                          retrieval_floor_gating, self.dev)
        self.plan = stream_plan.StreamPlan(self.capacity, self.k, strict_mode, verifier_floor_gating, verify,
                                           min_inliers, min_inlier_ratio)
        self.eng = _vit_engine(vit_state_dict, backbone, self.dev, vit_batch, vit_precise)
        self.K = _camera_matrix(torch, K, self.dev) if self.verify else None
        if self.verify:
            self.sp = SuperPointGPU(device=self.dev, max_num_keypoints=self.kp)
            self.lg = LightGlueGPU(device=self.dev)
            # every keyframe's SuperPoint features, extracted once when it arrives
            self.feats = lg_pairs.FeatureTable(self.capacity, self.kp, self.dev)
        self.h_kpcount = np.zeros(self.capacity, np.int32)
        self.frame_shape = None
        # ordered pairs that have gone through RANSAC, ever: no pair does twice
        self.ransac_pairs = 0
        self.last_append = {}
        # a list here makes append() record a timed HIP event after each stage: (stage, event)
        # pairs, the stage being what ran since the previous event (tools/bench_streaming_gate.py)
        self.stage_events = None

    def _mark(self, stage):
        if self.stage_events is not None:
            e = self.torch.cuda.Event(enable_timing=True)
            e.record()
            self.stage_events.append((stage, e))

    @property
    def n(self):
        return self.plan.n

    def lists(self):
        """The retrieval lists on the device (StreamingKnn.lists)."""
        return self.knn.lists()

    def report(self):
        """DeviceGate.step()'s counts on the keyframes seen so far."""
        return self.plan.counts()

    def pair_results(self):
        """The live verified ordered pairs, sorted by (a, b): gate_plan.pair_records' form."""
        return self.plan.pair_results()

    def append(self, frames, timestamps, floor_labels):
        """frames uint8 [B, H, W, C] on the device, their timestamps and floor labels.  Runs the
        ViT and SuperPoint on the new frames only, updates every retrieval list, brings the
        changed rows to the host in one transfer, and verifies the ordered pairs that are new.
        Returns the cumulative counts plus 'appended', 'new_pairs_verified', 'pairs_evicted',
        'new_closures' (arrays a, b, similarity, matches, inliers, and pose f64 [P, 4, 4] when K
        is given, of the pairs every stage newly accepts) and 'retracted' (arrays a, b of the
        pairs accepted earlier whose entry a better match has now pushed out)."""
        torch, dev, k = self.torch, self.dev, self.k
        # everything is checked before the first launch
        try:
            frames = _native.device_frames(frames)
        except TypeError as e:
            raise ValueError(str(e))
        B = int(frames.shape[0])
        ts = np.asarray(timestamps, np.float64).reshape(-1)
        labels = gate_plan.label_list(floor_labels)
        if B < 1 or len(ts) != B or len(labels) != B:
            raise ValueError(f"{B} frames, {len(ts)} timestamps, {len(labels)} floor labels")
        n_old, n_new = self.n, self.n + B
        if n_new > self.capacity:
            raise ValueError(f"appending {B} keyframes to {n_old} exceeds the capacity {self.capacity}")
        if self.frame_shape is None:
            self.frame_shape = tuple(frames.shape[1:])
        elif tuple(frames.shape[1:]) != self.frame_shape:
            raise ValueError(f"frames are {tuple(frames.shape[1:])}, the first append's were {self.frame_shape}")
        codes, has = self.plan.add_labels(labels)

        # 1-3: descriptors and SuperPoint features of the new frames, then the kNN update
        self._mark("start")
        desc = torch.empty(B, self.embed, dtype=torch.float32, device=dev)
        self.eng.forward_into(frames, desc, None)
        self._mark("vit")
        if self.verify:
            self.feats.fill(self.sp, frames, n_old, self.sp_batch)
        self._mark("superpoint")
        inserted, ev_idx, n_ev = self.knn.append(desc, torch.from_numpy(ts).to(dev), torch.from_numpy(codes).to(dev),
                                                 torch.from_numpy(has).to(dev))
        self._mark("knn_append")

        # 4: which old rows changed (4 B per old row), then those rows and the new ones in one
        # transfer (stream_plan.PACKED_COLUMNS)
        rows = self.plan.changed_rows(inserted.cpu().numpy(), n_old, n_new)
        rt = torch.from_numpy(rows).to(dev)
        fresh = rt >= n_old
        old = rt.clamp(max=max(n_old - 1, 0))
        i32 = lambda x: x.to(torch.int32)  # noqa: E731
        nev = torch.where(fresh, 0, n_ev[old]) if n_old else torch.zeros_like(rt, dtype=torch.int32)
        ev = (torch.where(fresh[:, None], -1, ev_idx[old]) if n_old
              else torch.full((len(rows), k), -1, dtype=torch.int32, device=dev))
        kpc = self.feats.cnt.view(-1)[rt] if self.verify else torch.zeros_like(rt, dtype=torch.int32)
        cols = {"idx": self.knn.idx[rt], "sim": self.knn.sim[rt].view(torch.int32), "valid": i32(self.knn.valid[rt]),
                "count": self.knn.count[rt], "n_evicted": i32(nev), "evicted": i32(ev), "kp_count": i32(kpc)}
        packed = torch.cat([cols[name] if wide else cols[name][:, None]
                            for name, wide in stream_plan.PACKED_COLUMNS], 1)
        r = stream_plan.unpack(packed.cpu().numpy(), k)
        self.h_kpcount[n_old:n_new] = r["kp_count"][len(rows) - B:]
        up = self.plan.update(n_new, rows, r["idx"], r["sim"], r["valid"], r["count"], r["n_evicted"], r["evicted"])
        self._mark("transfer_and_plan")

        # 5-6: LightGlue under the canonical orientation and RANSAC on the new ordered pairs
        # only, in DeviceGate's chunks; their results come to the host in one transfer
        va, vb = up["verify"]
        closures = {"a": va[:0], "b": vb[:0], "similarity": np.zeros(0, np.float32),
                    "matches": np.zeros(0, np.int32), "inliers": np.zeros(0, np.int32)}
        if self.K is not None:
            closures["pose"] = np.zeros((0, 4, 4), np.float64)
        if len(va):
            n_m, n_i, pose = self._verify_pairs(va, vb)
            _, acc = self.plan.record(va, vb, n_m, n_i, pose)
            s = self.plan._slots(va[acc].astype(np.int64), vb[acc].astype(np.int64))
            closures.update(a=va[acc], b=vb[acc], similarity=self.plan.sim[va[acc], s], matches=n_m[acc],
                            inliers=n_i[acc])
            if pose is not None:
                closures["pose"] = pose[acc]
        self._mark("results_and_plan")
        out = self.plan.counts()
        out.update(appended=B, new_pairs_verified=len(va), pairs_evicted=len(up["evicted"][0]), new_closures=closures,
                   retracted={"a": up["retracted"][0], "b": up["retracted"][1]})
        # what this append did, for tests and tools: the ordered pairs it sent through RANSAC
        self.last_append = {"changed_rows": len(rows), "new_pairs": len(up["new"][0]), "verified": (va, vb)}
        return out

    def _verify_pairs(self, pa, pb):
        """(matches int32 [P], inliers int32 [P], pose f64 [P, 4, 4] or None) of the ordered
        pairs (pa, pb): LightGlue once per unordered (min, max) pair and mlg_lg_orient_matches,
        then one RANSAC per ordered pair, as DeviceGate._verify_lightglue runs them (the same
        lg_pairs.oriented_matches, over the keyframes seen)."""
        torch = self.torch
        kp_all = self.feats.kp.view(self.capacity, self.kp, 2)
        ds_all = self.feats.ds.view(self.capacity, self.kp, 256)
        parts = []
        for sel, m, n in lg_pairs.oriented_matches(self.lg, kp_all, ds_all, self.h_kpcount, pa, pb, max(self.n, 1),
                                                   self.lg_chunk):
            self._mark("lightglue")
            _, _, inl, pose, _ = lg_pairs.ransac_pairs(self.K, kp_all, m, n, np.asarray(pa[sel], np.int32),
                                                       np.asarray(pb[sel], np.int32))
            self._mark("ransac")
            self.ransac_pairs += len(sel)
            parts.append((sel, n, inl, pose))
        sel = np.concatenate([p[0] for p in parts])
        cols = [torch.cat([p[1] for p in parts]).double()[:, None], torch.cat([p[2] for p in parts]).double()[:, None]]
        has_pose = parts[0][3] is not None
        if has_pose:
            cols.append(torch.cat([p[3] for p in parts]).view(-1, 16))
        # the chunks' sel together are a permutation of the pairs: back to (pa, pb)'s order
        host = torch.cat(cols, 1).cpu().numpy()[np.argsort(sel)]
        pose = host[:, 2:].reshape(-1, 4, 4) if has_pose else None
        return host[:, 0].astype(np.int32), host[:, 1].astype(np.int32), pose
