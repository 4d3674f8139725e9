"""Visual place recognition: the drop-in mirror of scripts/semantic_gating/place_recognition.py.

Same class names, constructor signatures, dataclasses, return types and error
behaviour as the reference; the compute runs on the mlgate HIP kernels:

  * CricaVPR -> DINOv2 ViT-B/14 + GeM on MI355X (mlgate.vit.VitB14); ONE forward per
    keyframe feeds both the descriptor and the local-feature cache (the reference runs
    the same forward twice, place_recognition.py:765/777); opt-in
    (MLGATE_CRICAVPR_NATIVE=1) the 10752-dim descriptor the class declares, from the same
    forward: mlgate.crica.
  * AnyLoc  -> the same ViT at 518^2 with mean pooling and unswapped channels
    (place_recognition.py:467-505); opt-in (MLGATE_ANYLOC_NATIVE=1) the VLAD descriptor
    the class declares, over the same tokens: mlgate.anyloc.
  * retrieval (find_loop_closures / query / pairwise similarities / cross-correlation
    rerank) -> mlg_knn_gate / mlg_knn_query / mlg_xcorr_score.
  * MixVPR / SALAD -> the reference resolves both to a torchvision ResNet-50 GAP
    fallback (place_recognition.py:241-306, 370-378); here that network runs on the
    GPU (mlgate.resnet: Pillow-exact resize, HIP stem, MFMA bottlenecks, GAP, zero-pad).
    SALAD's native branch (DINOv2 + Sinkhorn aggregation) is opt-in: mlgate.salad;
    so is MixVPR's (cropped ResNet-50 + feature mixer at 320^2): mlgate.mixvpr.

Weights: the hub checkpoint cannot be fetched offline.  ``pretrained_path`` (or
MLGATE_DINOV2_WEIGHTS) may point at a local hub-format dinov2_vitb14 state_dict;
otherwise seeded synthetic weights are used and a warning says so.
"""
import os
import warnings
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Tuple, Union

import numpy as np

from . import _native, weights
from .gate_plan import floor_codes  # the floor check's equality codes, stated once in gate_plan


@dataclass
class PlaceMatch:
    """A retrieved (query, match) pair; ``is_valid`` is the floor-gate decision."""
    query_idx: int
    match_idx: int
    similarity: float
    query_timestamp: Optional[float] = None
    match_timestamp: Optional[float] = None
    is_valid: bool = True


@dataclass
class PlaceDescriptor:
    """One database entry: global descriptor plus its timestamp / floor label."""
    timestamp: float
    descriptor: np.ndarray
    image_path: Optional[str] = None
    floor_label: Optional[int] = None


def _entries(descs, timestamps, floor_labels=None, image_paths=None):
    """One PlaceDescriptor per row of ``descs``."""
    return [PlaceDescriptor(timestamp=timestamps[i], descriptor=d,
                            image_path=None if image_paths is None else image_paths[i],
                            floor_label=None if floor_labels is None else floor_labels[i])
            for i, d in enumerate(descs)]


def _warn_synthetic(source, text):
    """Warn with ``text``, at the caller's line, when a weights source says the weights are
    seeded, not a checkpoint's."""
    if source.startswith("synthetic"):
        warnings.warn(text, stacklevel=2)


def _check_vitb14_head(backbone):
    if backbone != 'dinov2_vitb14':
        raise ValueError(f"{backbone}: the native branch's head is 768 wide, only the dinov2_vitb14 backbone has "
                         "MI355X kernels for it")


class _NativeSwitch:
    """The rule of every opt-in native branch: ``.native = None`` lets the environment variable
    ``_native_env`` decide ("1" selects the branch); True / False force it."""

    _native_env = None
    native = None

    def _native_selected(self):
        return self.native if self.native is not None else os.environ.get(self._native_env) == "1"


def _torch():
    import torch
    return torch


def _device_frames(images, device):
    """uint8 [B, H, W, C] on the device from a device / host tensor or a list of images."""
    torch = _torch()
    if isinstance(images, torch.Tensor):
        t = images if images.dim() == 4 else images.unsqueeze(-1)
        if t.dtype != torch.uint8:
            raise ValueError("frames must be uint8")
        return t.to(device).contiguous()
    return torch.from_numpy(_as_frames(images)).to(device)


def _as_frames(images):
    """List / array of HxW[xC] uint8 images (one size) -> contiguous uint8 [B, H, W, C]."""
    arrs = [np.asarray(im) for im in images]
    if not arrs:
        raise ValueError("no images")
    if any(a.shape != arrs[0].shape for a in arrs):
        raise ValueError("all images of a batch must have the same shape")
    batch = np.stack(arrs).astype(np.uint8, copy=False)
    if batch.ndim == 3:
        batch = batch[..., None]
    return np.ascontiguousarray(batch)


class BasePlaceRecognition:
    """Descriptor database + GPU retrieval shared by every VPR method."""

    def __init__(self, descriptor_dim: int = 4096, device: str = 'cuda'):
        self.descriptor_dim = descriptor_dim
        self.device = device
        self.model = None
        self.descriptors: List[PlaceDescriptor] = []

    # ---------------------------------------------------------- extraction
    def extract_descriptor(self, image: np.ndarray) -> np.ndarray:
        raise NotImplementedError

    def extract_descriptors(self, images) -> np.ndarray:
        """Batched extraction (mlgate extension): [B, D] float32."""
        return np.stack([self.extract_descriptor(im) for im in images])

    def add_image(self, image: np.ndarray, timestamp: float, floor_label: Optional[int] = None,
                  image_path: Optional[str] = None) -> PlaceDescriptor:
        entry = PlaceDescriptor(timestamp=timestamp, descriptor=self.extract_descriptor(image),
                                image_path=image_path, floor_label=floor_label)
        self.descriptors.append(entry)
        return entry

    def add_images(self, images, timestamps, floor_labels=None, image_paths=None) -> List[PlaceDescriptor]:
        """Batched add_image (mlgate extension): one device batch instead of N calls."""
        out = _entries(self.extract_descriptors(images), timestamps, floor_labels, image_paths)
        self.descriptors.extend(out)
        return out

    # ---------------------------------------------------------- database
    def build_descriptor_matrix(self) -> np.ndarray:
        if not self.descriptors:
            return np.array([])
        return np.vstack([d.descriptor for d in self.descriptors])

    def _device_matrix(self):
        """Device float32 [N, D] mirror of ``self.descriptors``.  Callers may append to (or
        replace entries of) the public list directly, as the reference allows
        (place_recognition.py:1020); the mirror tracks the descriptor arrays by identity
        and uploads only rows whose array object changed (appends upload only the new
        rows).  In-place edits of a descriptor array's values are not seen: replace the
        PlaceDescriptor (or its array) instead."""
        torch = _torch()
        dev = _native.require_device(self.device)
        arrs = [d.descriptor for d in self.descriptors]
        ids = [id(a) for a in arrs]
        m = getattr(self, '_mirror', None)
        D = int(np.asarray(arrs[0]).size) if arrs else 0
        if m is None or m['dev'] != dev or m['D'] != D or m['buf'].shape[0] < len(arrs):
            cap = max(len(arrs), 64, 0 if m is None else 2 * m['buf'].shape[0])
            buf = torch.empty(cap, D, dtype=torch.float32, device=dev)
            m = self._mirror = {'dev': dev, 'D': D, 'buf': buf, 'ids': [], 'keep': []}
        old = m['ids']
        stale = [i for i in range(len(ids)) if i >= len(old) or old[i] != ids[i]]
        if stale:
            lo = stale[0]
            if len(stale) == len(ids) - lo:  # one contiguous tail: a single upload
                rows = np.ascontiguousarray(np.stack([np.asarray(a, np.float32).reshape(-1) for a in arrs[lo:]]))
                m['buf'][lo:len(ids)].copy_(torch.from_numpy(rows))
            else:
                for i in stale:
                    m['buf'][i].copy_(torch.from_numpy(np.ascontiguousarray(arrs[i], dtype=np.float32).reshape(-1)))
        m['ids'] = ids
        m['keep'] = arrs  # hold the arrays so their ids stay unique while mirrored
        return m['buf'][:len(ids)], dev

    def compute_all_pairwise_similarities(self) -> np.ndarray:
        """N x N cosine similarities (float32), computed on the device."""
        if not self.descriptors:
            return np.array([])
        from . import retrieval
        X, _ = self._device_matrix()
        return retrieval.pairwise_similarities(X).cpu().numpy()

    def _compute_similarity(self, query: np.ndarray, database: np.ndarray) -> np.ndarray:
        torch = _torch()
        from . import retrieval
        dev = _native.require_device(self.device)
        db = torch.from_numpy(np.ascontiguousarray(database, dtype=np.float32)).to(dev)
        q = torch.from_numpy(np.ascontiguousarray(np.asarray(query, np.float32).reshape(1, -1))).to(dev)
        return retrieval.similarity(q, db)[0].cpu().numpy()

    def query(self, image: np.ndarray, timestamp: Optional[float] = None, k: int = 5,
              min_time_gap: float = 10.0) -> List[PlaceMatch]:
        """Top-k database entries for a new image (the query is not added)."""
        if not self.descriptors:
            return []
        torch = _torch()
        from . import retrieval
        qd = self.extract_descriptor(image)
        db, dev = self._device_matrix()
        t_db = torch.tensor([float(d.timestamp) for d in self.descriptors], dtype=torch.float64, device=dev)
        tq = torch.tensor([float('nan') if timestamp is None else float(timestamp)], dtype=torch.float64,
                          device=dev)
        q = torch.from_numpy(np.asarray(qd, np.float32).reshape(1, -1)).to(dev)
        kk = max(1, min(k, len(self.descriptors)))
        idx, sim, cnt = retrieval.knn_query(db, q, t_db, tq, min_time_gap if timestamp is not None else 0.0, kk)
        c = int(cnt[0]) if k > 0 else 0
        idx, sim = idx[0, :c].cpu().numpy(), sim[0, :c].cpu().numpy()
        n = len(self.descriptors)
        return [PlaceMatch(query_idx=n, match_idx=int(j), similarity=float(s), query_timestamp=timestamp,
                           match_timestamp=self.descriptors[int(j)].timestamp) for j, s in zip(idx, sim)]


class _ResNetFallback(_NativeSwitch, BasePlaceRecognition):
    """MixVPR / SALAD: what the reference executes is a torchvision ResNet-50 GAP
    (place_recognition.py:248-306) -- the MixVPR / SALAD packages are never importable
    under the names it tries, so every call lands in ``_load_fallback_model``.  Here
    that network runs on the GPU (mlgate.resnet, HIP kernels + bf16 MFMA GEMMs).

    A subclass names its opt-in native branch: ``_native_env``, the attribute that holds the
    native engine (``_native_attr``), ``_build_native()`` (its dimension / backbone checks and
    its engine constructor), the warning when that engine runs on seeded weights and, for
    SALAD, the reference's warning before the fallback loads."""

    _native_attr = None
    _synthetic_warning = None
    _fallback_warning = None

    def __init__(self, descriptor_dim, device, pretrained_path=None):
        super().__init__(descriptor_dim, device)
        self.pretrained_path = pretrained_path
        self._model_loaded = False
        setattr(self, self._native_attr, None)

    def _build_native(self):
        raise NotImplementedError

    def _load_model(self):
        if self._model_loaded:
            return
        native = self._native_selected()
        if native:
            engine = self._build_native()
            setattr(self, self._native_attr, engine)
            _warn_synthetic(engine.weights_source, self._synthetic_warning)
        else:
            if self._fallback_warning:
                warnings.warn(self._fallback_warning)
            from .resnet import ResNet50GPU
            self._net = ResNet50GPU(device=self.device)
            _warn_synthetic(self._net.weights_source,
                            "ImageNet ResNet-50 weights are not available offline; using seeded synthetic resnet50 "
                            "weights (set MLGATE_RESNET50_WEIGHTS to a local torchvision checkpoint).")
        self._model_loaded = True
        self._is_fallback = not native

    def extract_descriptors(self, images) -> np.ndarray:
        self._load_model()
        engine = getattr(self, self._native_attr)
        if engine is None:
            frames = _device_frames(images, self._net.device)
            return self._net.forward_device(frames, self.descriptor_dim).cpu().numpy()
        return engine.forward(_device_frames(images, engine.device)).cpu().numpy()

    def extract_descriptor(self, image: np.ndarray) -> np.ndarray:
        return self.extract_descriptors([image])[0]


class MixVPR(_ResNetFallback):
    """place_recognition.py:209-332.  By default what the reference executes: the ``mixvpr``
    package does not import, so the ResNet-50 GAP fallback runs (:241-306).
    ``MLGATE_MIXVPR_NATIVE=1`` (or ``.native = True``) selects the model its native branch
    names (:227-239): MixVPRModel(backbone='resnet50', out_dim=4096), the cropped ResNet-50
    + feature-mixer head at 320 x 320 on the GPU (mlgate.mixvpr, csrc/mixvpr.hip); weights
    from ``pretrained_path`` / MLGATE_MIXVPR_WEIGHTS, else seeded synthetic ones."""

    _native_env, _native_attr = "MLGATE_MIXVPR_NATIVE", "_mix"
    _synthetic_warning = ("MixVPR weights not configured (pretrained_path / MLGATE_MIXVPR_WEIGHTS); using seeded "
                          "synthetic weights")

    def __init__(self, backbone: str = 'resnet50', descriptor_dim: int = 4096, device: str = 'cuda',
                 pretrained_path: Optional[str] = None):
        super().__init__(descriptor_dim, device, pretrained_path)
        self.backbone_name = backbone

    def _build_native(self):
        from .mixvpr import DESC_DIM, MixVprGPU
        if self.backbone_name != 'resnet50':
            raise ValueError(f"native MixVPR: only the resnet50 backbone has MI355X kernels, not {self.backbone_name}")
        if self.descriptor_dim != DESC_DIM:
            raise ValueError(f"native MixVPR produces {DESC_DIM}-dim descriptors, not {self.descriptor_dim}")
        return MixVprGPU(device=self.device, pretrained_path=self.pretrained_path)


class SALAD(_ResNetFallback):
    """place_recognition.py:335-410.  By default what the reference executes: the
    ``salad`` package does not import, so SALAD warns and runs the MixVPR fallback
    (:370-378).  ``MLGATE_SALAD_NATIVE=1`` (or ``.native = True``) selects the model its
    native branch names (:357-368): serizba/salad's DINOv2 ViT-B/14 + optimal-transport
    aggregator (64 clusters x 128 + 256 token dims = 8448) on the GPU (mlgate.salad,
    csrc/salad.hip); weights from ``pretrained_path`` / MLGATE_SALAD_WEIGHTS, else seeded
    synthetic ones."""

    _native_env, _native_attr = "MLGATE_SALAD_NATIVE", "_salad"
    _synthetic_warning = ("SALAD weights not configured (pretrained_path / MLGATE_SALAD_WEIGHTS); using seeded "
                          "synthetic weights")
    _fallback_warning = "SALAD not installed. Using MixVPR fallback. For SALAD: pip install salad-vpr"

    def __init__(self, descriptor_dim: int = 8448, device: str = 'cuda', pretrained_path: Optional[str] = None):
        super().__init__(descriptor_dim, device, pretrained_path)

    def _build_native(self):
        from .salad import DESC_DIM, SaladGPU
        if self.descriptor_dim != DESC_DIM:
            raise ValueError(f"native SALAD produces {DESC_DIM}-dim descriptors, not {self.descriptor_dim}")
        return SaladGPU(device=self.device, pretrained_path=self.pretrained_path)


class _DinoEngineMixin(_NativeSwitch):
    """Lazy DINOv2 engine construction shared by CricaVPR and AnyLoc: ``backbone`` is one of
    dinov2_vits14 / dinov2_vitb14 / dinov2_vitl14 (feat_dim 384 / 768 / 1024,
    place_recognition.py:594-602)."""

    _image_size = 322
    _pool = "gem"
    _swap_rb = True

    def _dino_state_dict(self, setting):
        """The backbone's state dict; seeded weights come with a warning that names ``setting``."""
        sd, source = weights.resolve_state_dict(getattr(self, 'pretrained_path', None), backbone=self.backbone_name)
        _warn_synthetic(source, "DINOv2 hub weights are not available offline; using seeded synthetic "
                                f"{self.backbone_name} weights (set {setting} to a local hub checkpoint for real "
                                "descriptors).")
        return sd

    def _engine(self):
        if getattr(self, '_vit', None) is None:
            from .vit import engine_for
            embed = weights.backbone_config(self.backbone_name)[0]  # ValueError lists the supported names
            sd = self._dino_state_dict("pretrained_path or MLGATE_DINOV2_WEIGHTS")
            # the split-bf16 forward (VitB14's default): descriptors within ~1e-11 of fp32,
            # so retrieval ranks as the fp32 reference does
            self._vit = engine_for(sd, self.backbone_name, device=self.device, image_size=self._image_size,
                                   pool=self._pool, swap_rb=self._swap_rb, precise=True)
            self.feat_dim = embed
            self._model_loaded = True
        return self._vit

    def _forward(self, images, with_local=False):
        eng = self._engine()
        return eng.forward(_device_frames(images, eng.device), with_local=with_local)

    def extract_descriptors(self, images) -> np.ndarray:
        return self._forward(images).cpu().numpy()

    def extract_descriptor(self, image: np.ndarray) -> np.ndarray:
        return self._forward([image])[0].cpu().numpy().flatten()


class AnyLoc(_DinoEngineMixin, BasePlaceRecognition):
    _native_env = "MLGATE_ANYLOC_NATIVE"
    _image_size = 518
    _pool = "mean"
    _swap_rb = False

    def __init__(self, backbone: str = 'dinov2_vitb14', descriptor_dim: int = 49152, device: str = 'cuda',
                 num_clusters: int = 64):
        super().__init__(descriptor_dim, device)
        self.backbone_name = backbone
        self.num_clusters = num_clusters
        self._model_loaded = False
        self._vit = None
        self._anyloc = None
        self._vocabulary = None

    def _check_native_dims(self):
        if self.num_clusters not in weights.VLAD_CLUSTERS:
            raise ValueError(f"native AnyLoc: num_clusters = {self.num_clusters} is not a multiple of 16 in 16..128 "
                             f"(descriptor_dim = {self.descriptor_dim})")
        if self.descriptor_dim != self.num_clusters * weights.VLAD_DIM:
            raise ValueError(f"native AnyLoc produces num_clusters x {weights.VLAD_DIM} = "
                             f"{self.num_clusters * weights.VLAD_DIM}-dim descriptors (num_clusters = "
                             f"{self.num_clusters}), not {self.descriptor_dim}")

    def _build_engine(self, vocabulary):
        self._check_native_dims()
        _check_vitb14_head(self.backbone_name)
        from .anyloc import AnyLocGPU
        sd = self._dino_state_dict("MLGATE_DINOV2_WEIGHTS")
        self.feat_dim = 768
        self._model_loaded = True
        return AnyLocGPU(sd, vocabulary, device=self.device, image_size=self._image_size)

    def _native_engine(self):
        """The AnyLocGPU engine when the native branch is selected, else None."""
        if not self._native_selected():
            return None
        if self._anyloc is None:
            self._check_native_dims()
            vocab = self._vocabulary
            if vocab is None:
                vocab, source = weights.resolve_vocabulary(None, self.num_clusters)
                _warn_synthetic(source, "AnyLoc vocabulary not configured (set_vocabulary / fit_vocabulary / "
                                        "MLGATE_ANYLOC_VOCAB); using a seeded synthetic vocabulary")
                self._vocabulary = vocab
            self._anyloc = self._build_engine(vocab)
        return self._anyloc

    def set_vocabulary(self, centers):
        """VLAD cluster centres [num_clusters, 768] for the native branch (mlgate extension)."""
        if hasattr(centers, 'detach'):
            centers = centers.detach().float().cpu().numpy()
        self._vocabulary = weights.check_vocabulary(centers, self.num_clusters)
        if self._anyloc is not None:
            self._anyloc.set_vocabulary(self._vocabulary)

    def fit_vocabulary(self, images, seed=0, max_iter=100):
        """Fit the VLAD vocabulary on the tokens of ``images`` (k-means on the device),
        install it and return the centres [num_clusters, 768] (mlgate extension)."""
        from .anyloc import fit_vocabulary
        eng = self._anyloc
        if eng is None:  # the engine needs some vocabulary to exist; the fit replaces it
            eng = self._build_engine(np.zeros((self.num_clusters, 768), np.float32))
        centers = fit_vocabulary((eng, _device_frames(images, eng.device)), self.num_clusters, seed, max_iter)
        self._anyloc = eng
        self.set_vocabulary(centers)
        return centers

    def _forward(self, images, with_local=False):
        eng = self._native_engine()
        if eng is None:
            return super()._forward(images, with_local)
        return eng.forward(_device_frames(images, eng.device))


class CricaVPR(_DinoEngineMixin, BasePlaceRecognition):
    _native_env = "MLGATE_CRICAVPR_NATIVE"

    def __init__(self, backbone: str = 'dinov2_vitb14', descriptor_dim: int = 10752, device: str = 'cuda',
                 pretrained_path: Optional[str] = None, use_reranking: bool = True):
        super().__init__(descriptor_dim, device)
        self.backbone_name = backbone
        self.pretrained_path = pretrained_path
        self.use_reranking = use_reranking
        self._model_loaded = False
        self._vit = None
        self._feature_cache = {}  # idx -> device float32 [1, 528, feat_dim]
        self.cross_image_group = 1  # images of a call that attend to each other (native branch)
        self._crica = None

    def _native_engine(self):
        """The CricaGPU engine when the native branch is selected, else None."""
        if not self._native_selected():
            return None
        if self._crica is None or self._crica.group != int(self.cross_image_group):
            if self.descriptor_dim != 10752:
                raise ValueError(f"native CricaVPR produces 14 x 768 = 10752-dim descriptors, not "
                                 f"{self.descriptor_dim}")
            _check_vitb14_head(self.backbone_name)
            from .crica import CricaGPU, check_group
            group = check_group(self.cross_image_group)
            if self._crica is not None:  # the group changed: the packed weights stay
                self._crica.group = group
                return self._crica
            sd, source = weights.resolve_crica_state_dict(self.pretrained_path)
            _warn_synthetic(source, "CricaVPR weights are not available offline; using seeded synthetic weights (set "
                                    "pretrained_path or MLGATE_CRICAVPR_WEIGHTS to a local CricaVPRNet checkpoint "
                                    "for real descriptors).")
            self._crica = CricaGPU(sd, device=self.device, image_size=self._image_size,
                                   max_batch=max(64, group), group=group)
            self.feat_dim = 768
            self._model_loaded = True
        return self._crica

    def _forward(self, images, with_local=False):
        eng = self._native_engine()
        if eng is None:
            return super()._forward(images, with_local)
        return eng.forward(_device_frames(images, eng.device), with_local=with_local)

    def extract_local_features(self, image: np.ndarray) -> np.ndarray:
        _, local = self._forward([image], with_local=True)
        return local.cpu().numpy()

    def _to_device_feats(self, f):
        torch = _torch()
        dev = self._engine().device if getattr(self, '_vit', None) is not None else _native.require_device(
            self.device)
        t = f if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32))
        t = t.to(dev, torch.float32)
        if t.dim() == 3:
            t = t.squeeze(0)
        return t.contiguous()

    def compute_cross_correlation_score(self, query_features, match_features) -> float:
        from . import retrieval
        return float(retrieval.xcorr_score(self._to_device_feats(query_features),
                                           self._to_device_feats(match_features)).item())

    def rerank_candidates(self, query_idx: int, candidates: List[Tuple[int, float]],
                          top_k: int = 5) -> List[Tuple[int, float]]:
        """place_recognition.py:714-757: 0.5 global + 0.5 cross-correlation, sorted
        (stable) by the combined score; every candidate of the query scored in ONE batched
        pass (mlg_xcorr_batch) instead of one correlation per candidate."""
        if not self.use_reranking or query_idx not in self._feature_cache:
            return candidates[:top_k]
        return self.rerank_candidates_batch({query_idx: candidates}, top_k)[query_idx]

    def rerank_candidates_batch(self, requests: Dict[int, List[Tuple[int, float]]],
                                top_k: int = 5) -> Dict[int, List[Tuple[int, float]]]:
        """rerank_candidates for many queries at once ({query_idx: [(match_idx,
        global_sim), ...]}): all (query, candidate) cross-correlation scores of all
        queries in one batched pass over the cached local features (one frame bank, no
        [L, L] matrix per pair), then the reference's combination and stable sort per query."""
        torch = _torch()
        pairs = [(q, j) for q, cands in requests.items() if self.use_reranking and q in self._feature_cache
                 for j, _ in cands if j in self._feature_cache]
        scores = {}
        if pairs:
            frames = sorted({i for p in pairs for i in p})
            pos = {f: k for k, f in enumerate(frames)}
            bank = torch.cat([self._to_device_feats(self._feature_cache[f])[None] for f in frames])
            dev = bank.device
            qa = torch.tensor([pos[q] for q, _ in pairs], dtype=torch.int32, device=dev)
            qb = torch.tensor([pos[j] for _, j in pairs], dtype=torch.int32, device=dev)
            sc = _native.ops().xcorr_batch(bank.contiguous(), qa, qb).cpu().numpy()
            scores = {p: float(v) for p, v in zip(pairs, sc)}
        out = {}
        for q, cands in requests.items():
            if not self.use_reranking or q not in self._feature_cache:
                out[q] = cands[:top_k]
                continue
            scored = [(j, 0.5 * g + 0.5 * scores[(q, j)]) if (q, j) in scores else (j, g) for j, g in cands]
            scored.sort(key=lambda x: x[1], reverse=True)
            out[q] = scored[:top_k]
        return out

    def _append(self, descs, local, timestamps, floor_labels, image_paths):
        out = _entries(descs, timestamps, floor_labels, image_paths)
        for i, entry in enumerate(out):
            self.descriptors.append(entry)
            if self.use_reranking:
                self._feature_cache[len(self.descriptors) - 1] = local[i:i + 1]
        return out

    def add_image(self, image: np.ndarray, timestamp: float, floor_label: Optional[int] = None,
                  image_path: Optional[str] = None) -> PlaceDescriptor:
        desc, local = self._forward([image], with_local=True)
        return self._append(desc.cpu().numpy(), local, [timestamp], [floor_label], [image_path])[0]

    def add_images(self, images, timestamps, floor_labels=None, image_paths=None) -> List[PlaceDescriptor]:
        desc, local = self._forward(images, with_local=True)
        return self._append(desc.cpu().numpy(), local, timestamps, floor_labels, image_paths)


_METHODS = {'mixvpr': MixVPR, 'salad': SALAD, 'anyloc': AnyLoc, 'cricavpr': CricaVPR}


class SemanticPlaceRecognition:
    """VPR database + floor-gated all-keyframes loop-closure retrieval."""

    def __init__(self, vpr_method: str = 'mixvpr', device: str = 'cuda', similarity_threshold: float = 0.5,
                 min_time_gap: float = 10.0):
        self.similarity_threshold = similarity_threshold
        self.min_time_gap = min_time_gap
        key = vpr_method.lower()
        if key not in _METHODS:
            raise ValueError(f"Unknown VPR method: {vpr_method}. Available: mixvpr, salad, anyloc, cricavpr")
        self.vpr = CricaVPR(device=device, use_reranking=True) if key == 'cricavpr' else _METHODS[key](device=device)

    def add_image(self, image: np.ndarray, timestamp: float, floor_label: int,
                  image_path: Optional[str] = None) -> PlaceDescriptor:
        return self.vpr.add_image(image, timestamp, floor_label, image_path)

    def add_images(self, images, timestamps, floor_labels, image_paths=None) -> List[PlaceDescriptor]:
        """Batched add_image (mlgate extension)."""
        return self.vpr.add_images(images, timestamps, floor_labels, image_paths)

    def find_loop_closures(self, enable_floor_gating: bool = True, k: int = 10) -> List[PlaceMatch]:
        descs = self.vpr.descriptors
        n = len(descs)
        if n < 2:
            return []
        torch = _torch()
        from . import retrieval
        if k <= 0:
            return []
        # a row ranks all n entries (its own included when min_time_gap <= 0): k beyond n
        # returns what argsort()[:k] returns, every candidate
        kk = min(k, n)
        X, dev = self.vpr._device_matrix()
        t = torch.tensor([float(d.timestamp) for d in descs], dtype=torch.float64, device=dev)
        codes, has = floor_codes([d.floor_label for d in descs])
        fl = torch.from_numpy(codes).to(dev)
        hf = torch.from_numpy(has).to(dev)
        out = retrieval.knn_gate(X, t, fl, hf, self.min_time_gap, self.similarity_threshold, kk,
                                 enable_floor_gating)
        q, m, sim, valid = retrieval.flatten_matches(*out)
        return [PlaceMatch(query_idx=int(i), match_idx=int(j), similarity=float(s),
                           query_timestamp=descs[int(i)].timestamp, match_timestamp=descs[int(j)].timestamp,
                           is_valid=bool(v)) for i, j, s, v in zip(q, m, sim, valid)]

    def get_statistics(self, matches: List[PlaceMatch]) -> Dict:
        if not matches:
            return {'total_matches': 0, 'valid_matches': 0, 'rejected_matches': 0, 'rejection_rate': 0.0}
        ok = [m.is_valid for m in matches]
        n_valid = sum(ok)
        n = len(matches)
        sims = [m.similarity for m in matches]
        return {
            'total_matches': n,
            'valid_matches': n_valid,
            'rejected_matches': n - n_valid,
            'rejection_rate': (n - n_valid) / n,
            'mean_similarity': np.mean(sims),
            'mean_valid_similarity': np.mean([s for s, v in zip(sims, ok) if v]) if n_valid > 0 else 0.0,
        }


def process_image_sequence(image_dir: Union[str, Path], timestamps: np.ndarray, floor_labels: np.ndarray,
                           vpr_method: str = 'mixvpr',
                           device: str = 'cuda') -> Tuple[SemanticPlaceRecognition, List[PlaceMatch]]:
    """Sorted *.png then *.jpg of a directory -> database -> floor-gated loop closures
    (place_recognition.py:936-991).

    Both kinds go through one mlgate.ingest.KeyframeStream and are added in device
    batches: PNG keyframes (what bag_utils.extract_images writes) are decoded on a host
    thread pool; *.jpg files are Huffman-decoded there and finished on the GPU (IDCT,
    upsampling, colour: libjpeg-turbo's integers, so cv2.imread's pixels).  A JPEG the
    native path declines is read by mlgate.ingest.jpeg_reader() (cv2.imread when OpenCV is
    installed, else Pillow's libjpeg decode; its ImportError is raised only then).  The
    database, warnings and matches are those of the reference's one-image-at-a-time loop."""
    from . import ingest
    image_dir = Path(image_dir)
    spr = SemanticPlaceRecognition(vpr_method=vpr_method, device=device)
    files = sorted(image_dir.glob('*.png')) + sorted(image_dir.glob('*.jpg'))
    if len(files) != len(timestamps):
        warnings.warn(f"Number of images ({len(files)}) != timestamps ({len(timestamps)}). Using minimum of both.")
    n = min(len(files), len(timestamps), len(floor_labels))
    files = files[:n]
    print(f"Processing {n} images with {vpr_method}...")
    for rows, frames in ingest.KeyframeStream(files, device=device):
        spr.add_images(frames, [timestamps[i] for i in rows], [int(floor_labels[i]) for i in rows],
                       [str(files[i]) for i in rows])
        for i in rows:
            if (i + 1) % 100 == 0:
                print(f"  Processed {i + 1}/{n} images")
    print("Finding loop closure candidates...")
    return spr, spr.find_loop_closures(enable_floor_gating=True)
