"""AnyLoc's native branch on the GPU (csrc/vlad.hip, mlgate/anyloc.py) against the float64
restatement (tests/anyloc_restatement.py).  Every bar is a reference-side quantity: the
float32 rounding floor e_f32, the label margin (float64 top-2 cosine gap) and e_flip are
computed from the restatement and the fp32 oracle, never from what the kernels return;
tests/test_anyloc_cpu.py asserts the fixtures' conditions."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import anyloc_restatement as R
from mlgate import _native
from mlgate.anyloc import AnyLocGPU, fit_vocabulary
from mlgate.vit import VitB14
from mlgate.vpr import AnyLoc, SemanticPlaceRecognition
from mlgate.weights import synthetic_state_dict, synthetic_vocabulary

pytestmark = pytest.mark.gpu


def _vlad(dev, tokens, centers):
    d, l = _native.ops().vlad(torch.from_numpy(np.ascontiguousarray(tokens)).to(dev), torch.from_numpy(centers).to(dev))
    return d.cpu().numpy(), l.cpu().numpy()


@pytest.fixture(scope="module")
def engine(dev):
    f = R.e2e_fixture()
    return AnyLocGPU(f["state_dict"], f["centers"], device=str(dev), max_batch=2)


# ------------------------------------------------------------ 1. the head on given tokens
@pytest.mark.parametrize("shape", R.HEAD_SHAPES)
def test_head_matches_float64(dev, shape):
    """Labels equal the restatement's wherever its top-2 cosine gap is >= 1e-5 (about 80x the
    f32-matmul error, 1.2e-7); below it at most 0.5 % of the tokens may differ.  With equal
    labels on the decided tokens, 1 - cos to float64 <= 8 e_f32 per frame."""
    B, P, K = shape
    tokens, centers = R.head_fixture(shape)
    desc, labels = _vlad(dev, tokens, centers)
    assert desc.shape == (B, K * 768) and desc.dtype == np.float32 and labels.shape == (B, P)
    assert labels.dtype == np.int32 and labels.min() >= 0 and labels.max() < K
    assert np.all(np.isfinite(desc))
    assert np.all(np.abs(np.linalg.norm(desc.astype(np.float64), axis=1) - 1) <= 1e-5)
    if P > 1:
        assert labels[0, 1] == 0  # the zero token
    differ = 0
    for b in range(B):
        ref_l, gap, _ = R.assign(tokens[b], centers)
        decided = gap >= R.GAP_DECIDED
        assert np.array_equal(labels[b][decided], ref_l[decided]), (b, np.flatnonzero(labels[b] != ref_l))
        differ += int(np.sum(labels[b] != ref_l))
        ref = R.vlad(tokens[b], centers, labels[b])  # the GPU's choice on the undecided tokens
        e_f32 = R.one_minus_cos(R.vlad_f32(tokens[b], centers, labels[b]), ref)
        err = R.one_minus_cos(desc[b], ref)
        print(f"{shape} frame {b}: 1 - cos {err:.3e}, e_f32 {e_f32:.3e}, ratio {err / e_f32:.2f}; "
              f"undecided {int((~decided).sum())}, differing {int(np.sum(labels[b] != ref_l))}")
        assert err <= 8 * e_f32, (b, err, e_f32)
        empty = np.bincount(labels[b], minlength=K) == 0
        assert np.all(desc[b].reshape(K, 768)[empty] == 0)
    assert differ <= R.UNDECIDED_CAP * B * P


# ------------------------------------------------------------ 2. independence
def test_rows_are_independent_and_repeatable(dev):
    tokens, centers = R.head_fixture((3, 1368, 64))
    d3, l3 = _vlad(dev, tokens, centers)
    again = _vlad(dev, tokens, centers)
    assert np.array_equal(d3, again[0]) and np.array_equal(l3, again[1])
    d1, l1 = _vlad(dev, tokens[:1], centers)
    assert np.array_equal(d1[0], d3[0]) and np.array_equal(l1[0], l3[0])
    moved = tokens[[2, 1, 0]]
    dm, lm = _vlad(dev, moved, centers)
    assert np.array_equal(dm[2], d3[0]) and np.array_equal(lm[2], l3[0])
    assert np.array_equal(dm[0], d3[2]) and np.array_equal(lm[0], l3[2])
    # an odd token count: frame 1 of a [3, 65] batch alone and in place
    t65, c65 = R.head_fixture((2, 65, 64))
    both, one = _vlad(dev, t65, c65), _vlad(dev, t65[1:], c65)
    assert np.array_equal(both[0][1], one[0][0]) and np.array_equal(both[1][1], one[1][0])


def test_token_offsets_past_2_31_bytes(dev):
    """Two frames of 350,100 tokens: frame 1 spans byte offsets 1.08 - 2.15 GB of the token
    tensor, across 2^31.  Its labels and descriptor equal those of the frame alone."""
    P, K = 350_100, 16
    g = torch.Generator(device=dev).manual_seed(5)
    tokens = torch.randn(2, P, 768, device=dev, generator=g)
    assert tokens.numel() * 4 > 2 ** 31 and P * 768 * 4 < 2 ** 31
    centers = torch.from_numpy(R.head_fixture((1, 1, K))[1]).to(dev)
    d2, l2 = _native.ops().vlad(tokens, centers)
    d1, l1 = _native.ops().vlad(tokens[1:].clone(), centers)
    assert torch.equal(l2[1], l1[0]) and torch.equal(d2[1], d1[0])
    assert torch.equal(torch.bincount(l2[1].long(), minlength=K) > 0, d2[1].view(K, 768).abs().sum(1) > 0)
    assert abs(float(d2[1].double().norm()) - 1) <= 1e-5


# ------------------------------------------------------------ 3. composition
def test_forward_is_vit_tokens_then_vlad(dev, engine):
    f = R.e2e_fixture()
    frames = torch.from_numpy(f["frames"][:2]).to(dev)
    got = engine.forward(frames)
    vit = VitB14(f["state_dict"], device=str(dev), image_size=518, pool="mean", swap_rb=False)
    toks = vit.forward(frames, with_local=True)[1]
    assert tuple(toks.shape) == (2, 1368, 768)
    assert torch.equal(engine.tokens(frames), toks)
    assert torch.equal(got, engine.vlad(toks))
    one = AnyLocGPU(f["state_dict"], f["centers"], device=str(dev), max_batch=1)
    assert torch.equal(one.forward(frames), got)


# ------------------------------------------------------------ 4. end to end
def test_descriptor_against_the_fp32_oracle(dev, engine):
    """One 480 x 640 frame through AnyLocGPU.forward against VLAD (float64) over the fp32
    oracle's tokens, vocabulary fitted by the restatement.  F = tokens whose float64 top-2
    gap is < 1e-4 (at most 1 % of 1368): labels must agree outside F, and 1 - cos must be
    within e_flip + 8 e_f32, e_flip the oracle descriptor's own change when F moves to the
    second-best clusters."""
    f = R.e2e_fixture()
    frames = torch.from_numpy(f["frames"][:1]).to(dev)
    desc = engine.forward(frames).cpu().numpy()[0]
    labels = engine.vlad(engine.tokens(frames), with_labels=True)[1].cpu().numpy()[0]
    out = ~f["F"]
    err = R.one_minus_cos(desc, f["ref"])
    print(f"|F| {int(f['F'].sum())}, labels differing {int(np.sum(labels != f['labels']))}, 1 - cos {err:.3e}, "
          f"e_flip {f['e_flip']:.3e}, e_f32 {f['e_f32']:.3e}")
    assert desc.shape == (64 * 768,) and np.all(np.isfinite(desc))
    assert abs(np.linalg.norm(desc.astype(np.float64)) - 1) <= 1e-5
    assert np.array_equal(labels[out], f["labels"][out]), np.flatnonzero(labels != f["labels"])
    assert err <= f["e_flip"] + 8 * f["e_f32"]


# ------------------------------------------------------------ 5. k-means
def test_fit_vocabulary_matches_the_lloyd_restatement(dev):
    x = R.planted_mixture()
    ref_c, ref_l, ref_n, _ = R.kmeans(x, 16, R.KMEANS_SEED)
    xd = torch.from_numpy(x).to(dev)
    c, info = fit_vocabulary(xd, 16, seed=R.KMEANS_SEED, return_info=True)
    assert c.shape == (16, 768) and c.dtype == np.float32
    assert info["n_iter"] == ref_n
    assert np.array_equal(info["labels"], ref_l)
    assert np.array_equal(info["counts"], np.bincount(ref_l, minlength=16))
    floor = np.abs(R.kmeans_update_f32(x, ref_l, ref_c) - ref_c).max()
    err = np.abs(c.astype(np.float64) - ref_c).max()
    print(f"centres max abs error {err:.3e}, f32 floor {floor:.3e}, ratio {err / floor:.2f}")
    assert err <= 8 * floor
    c2, info2 = fit_vocabulary(xd, 16, seed=R.KMEANS_SEED, return_info=True)
    assert np.array_equal(c, c2) and np.array_equal(info["labels"], info2["labels"])
    assert np.array_equal(fit_vocabulary(xd.reshape(2, 1000, 768), 16, seed=R.KMEANS_SEED), c)
    assert fit_vocabulary(xd, 16, seed=R.KMEANS_SEED, max_iter=1, return_info=True)[1]["n_iter"] == 1


def test_kmeans_more_clusters_than_directions(dev):
    """K = 32 over 16 planted directions, then one step with 16 centres nothing is nearest to:
    they keep their values bit for bit, with count 0."""
    x = R.planted_mixture()
    xd = torch.from_numpy(x).to(dev)
    c, info = fit_vocabulary(xd, 32, seed=R.KMEANS_SEED, return_info=True)
    assert c.shape == (32, 768) and np.all(np.isfinite(c)) and info["counts"].sum() == 2000
    assert np.array_equal(c, fit_vocabulary(xd, 32, seed=R.KMEANS_SEED))
    ref_c, ref_l, _, _ = R.kmeans(x, 16, R.KMEANS_SEED)
    both = np.concatenate([ref_c, -ref_c]).astype(np.float32)  # cosine to -c_k is negative for every token
    cd = torch.from_numpy(both).to(dev)
    labels = torch.full((2000,), -1, dtype=torch.int32, device=dev)
    changed, counts = _native.ops().kmeans_step(xd, cd, labels)
    assert int(changed.item()) == 2000 and np.array_equal(labels.cpu().numpy(), ref_l)
    assert np.array_equal(counts.cpu().numpy(), np.concatenate([np.bincount(ref_l, minlength=16), np.zeros(16, int)]))
    out = cd.cpu().numpy()
    assert np.array_equal(out[16:], both[16:]) and np.all(np.isfinite(out))
    changed, _ = _native.ops().kmeans_step(xd, cd, labels)
    assert int(changed.item()) == 0


# ------------------------------------------------------------ 6. drop-in
def test_dropin_native_and_default(dev, monkeypatch):
    for v in ("MLGATE_ANYLOC_NATIVE", "MLGATE_ANYLOC_VOCAB", "MLGATE_DINOV2_WEIGHTS"):
        monkeypatch.delenv(v, raising=False)
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    m = AnyLoc(device=str(dev))
    m.native = True
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        d = m.extract_descriptor(img)
    msgs = [str(w.message) for w in rec]
    assert any("synthetic" in s and "vocabulary" in s for s in msgs), msgs
    assert d.shape == (49152,) and d.dtype == np.float32 and abs(np.linalg.norm(d.astype(np.float64)) - 1) <= 1e-5
    assert m.extract_descriptor(img[..., 0]).shape == (49152,)
    # BGRA: alpha is dropped.  Unlike MixVPR's 320-wide rows, a 518-wide row of 4 channels
    # ends cv2's vector pass at another pixel than one of 3 (resize_cv.h resize_vec_end), so
    # the last two columns may round differently from the BGR frame's: compare two alphas.
    bgra = np.concatenate([img, np.full((480, 640, 1), 255, np.uint8)], axis=-1)
    da = m.extract_descriptor(bgra)
    bgra[..., 3] = rng.integers(0, 256, (480, 640), dtype=np.uint8)
    assert da.shape == (49152,) and np.array_equal(m.extract_descriptor(bgra), da)
    assert abs(np.linalg.norm(da.astype(np.float64)) - 1) <= 1e-5
    two = m.extract_descriptors([img, img[::-1].copy()])
    assert two.shape == (2, 49152) and two.dtype == np.float32 and np.array_equal(two[0], d)

    # default (native unset, no environment variable): today's 768-dim mean pool
    f = AnyLoc(device=str(dev))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        df = f.extract_descriptor(img)
        vit = VitB14(synthetic_state_dict(0), device=str(dev), image_size=518, pool="mean", swap_rb=False)
    assert df.shape == (768,) and f._anyloc is None
    assert np.array_equal(df, vit.forward(torch.from_numpy(img[None]).to(dev)).cpu().numpy()[0])

    # set_vocabulary: the engine's forward on the same centres
    vocab = synthetic_vocabulary(64, seed=5)
    m.set_vocabulary(vocab)
    eng = AnyLocGPU(synthetic_state_dict(0), vocab, device=str(dev))
    frames = torch.from_numpy(np.stack([img, img[::-1].copy()])).to(dev)
    got = m.extract_descriptors(frames)
    assert np.array_equal(got, eng.forward(frames).cpu().numpy()) and not np.array_equal(got[0], d)


def test_dropin_fit_vocabulary_and_environment(dev, monkeypatch, tmp_path):
    monkeypatch.setenv("MLGATE_ANYLOC_NATIVE", "1")
    monkeypatch.delenv("MLGATE_ANYLOC_VOCAB", raising=False)
    rng = np.random.default_rng(4)
    imgs = list(rng.integers(0, 256, (2, 120, 160, 3), dtype=np.uint8))
    m = AnyLoc(device=str(dev))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        c = m.fit_vocabulary(imgs, seed=1, max_iter=3)
        d = m.extract_descriptors(imgs)
    assert not any("vocabulary" in str(w.message) for w in rec)  # a fitted vocabulary: no synthetic one
    assert c.shape == (64, 768) and c.dtype == np.float32 and np.all(np.isfinite(c))
    np.save(tmp_path / "vocab.npy", c)
    monkeypatch.setenv("MLGATE_ANYLOC_VOCAB", str(tmp_path / "vocab.npy"))
    e = AnyLoc(device=str(dev))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        de = e.extract_descriptors(imgs)
    assert not any("vocabulary" in str(w.message) for w in rec)
    assert np.array_equal(de, d)


# ------------------------------------------------------------ 7. retrieval at D = 49152
def test_retrieval_over_native_descriptors(dev, monkeypatch):
    """find_loop_closures(k = 3) and query over 12 native descriptors equal the oracle
    restatement tests/test_retrieval_gpu.py uses, run on the same descriptors on the host."""
    from oracle import retrieval as oret
    monkeypatch.setenv("MLGATE_ANYLOC_NATIVE", "1")
    monkeypatch.delenv("MLGATE_ANYLOC_VOCAB", raising=False)
    rng = np.random.default_rng(12)
    frames = list(rng.integers(0, 256, (13, 240, 320, 3), dtype=np.uint8))
    t = [15.0 * i for i in range(12)]
    floors = [i % 3 for i in range(12)]
    spr = SemanticPlaceRecognition("anyloc", device=str(dev), similarity_threshold=0.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spr.add_image(frames[0], t[0], floors[0])
        spr.add_images(frames[1:12], t[1:], floors[1:])
        X = spr.vpr.build_descriptor_matrix()
        assert X.shape == (12, 49152) and X.dtype == np.float32
        got = spr.find_loop_closures(k=3)
        ungated = spr.find_loop_closures(enable_floor_gating=False, k=3)
        qm = spr.vpr.query(frames[12], timestamp=200.0, k=4, min_time_gap=50.0)
        qd = spr.vpr.extract_descriptor(frames[12])
    ta, fl, hf = np.array(t), np.array(floors, np.int64), np.ones(12, np.uint8)
    # no float32 near tie decides the ranking: the candidates a row can return, and the first it does not
    S = oret.pairwise_similarities(X).astype(np.float64)
    for i in range(12):
        row = np.sort(S[i][np.abs(ta - ta[i]) >= spr.min_time_gap])[::-1][:4]
        assert np.all(row[:-1] - row[1:] >= 1e-5), (i, row)
    for matches, gating in ((got, True), (ungated, False)):
        rq, rm, rs, rv = oret.find_loop_closures(X, ta, fl, hf, spr.min_time_gap, 0.0, 3, gating)
        assert len(matches) == len(rq) > 0
        assert [m.query_idx for m in matches] == rq.tolist() and [m.match_idx for m in matches] == rm.tolist()
        assert [m.is_valid for m in matches] == rv.astype(bool).tolist()
        assert np.max(np.abs(np.array([m.similarity for m in matches]) - rs)) <= 4e-6
    assert any(not m.is_valid for m in got) and all(m.is_valid for m in ungated)
    ro, rs = oret.query(X, qd, ta, 200.0, 4, 50.0)
    full = np.sort(oret.query(X, qd, ta, 200.0, 12, 50.0)[1])[::-1][:5]
    assert np.all(full[:-1] - full[1:] >= 1e-5), full
    assert [m.match_idx for m in qm] == ro.tolist() and len(qm) == 4
    assert np.max(np.abs(np.array([m.similarity for m in qm]) - rs)) <= 4e-6


# ------------------------------------------------------------ 8. ABI
class _Vocab(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("abi_version", ctypes.c_uint32), ("centers", ctypes.c_void_p),
                ("num_clusters", ctypes.c_int)]


def test_abi_rejects_bad_arguments(dev):
    lib = _native.lib()
    EINVAL = -1
    B, P, K = 2, 65, 64
    tokens, centers = R.head_fixture((B, P, K))
    td, cd = torch.from_numpy(tokens).to(dev), torch.from_numpy(centers).to(dev)
    n = lib.mlg_vlad_workspace_bytes(B, P, K)
    assert n > 0 and lib.mlg_vlad_workspace_bytes(B, P, 24) == 0 and lib.mlg_vlad_workspace_bytes(B, 0, K) == 0
    assert lib.mlg_vlad_workspace_bytes(B, P, 144) == 0 and lib.mlg_kmeans_workspace_bytes(100, 8) == 0
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    desc = torch.full((B, K * 768), 7.0, device=dev)
    stream = _native.stream_of(dev)

    def call(v, tok=td.data_ptr(), wsp=ws.data_ptr(), nbytes=n, out=desc.data_ptr()):
        return lib.mlg_op_vlad(ctypes.byref(v), tok, B, P, wsp, nbytes, out, None, stream)

    def vocab(**kw):
        v = _Vocab(ctypes.sizeof(_Vocab), lib.mlg_abi_version(), cd.data_ptr(), K)
        for k, x in kw.items():
            setattr(v, k, x)
        return v

    # a foreign head is rejected before the rest of the struct is read (the pointer below is not one)
    assert call(vocab(struct_size=8, centers=0xdead0000)) == EINVAL
    assert call(vocab(struct_size=ctypes.sizeof(_Vocab) + 8, centers=0xdead0000)) == EINVAL
    assert call(vocab(abi_version=lib.mlg_abi_version() + 1, centers=0xdead0000)) == EINVAL
    assert lib.mlg_op_vlad(None, td.data_ptr(), B, P, ws.data_ptr(), n, desc.data_ptr(), None, stream) == EINVAL
    assert call(vocab(num_clusters=24)) == EINVAL
    assert call(vocab(num_clusters=0)) == EINVAL
    assert call(vocab(centers=None)) == EINVAL
    assert call(vocab(), nbytes=n - 1) == EINVAL
    assert call(vocab(), wsp=None) == EINVAL
    assert call(vocab(), tok=None) == EINVAL
    assert call(vocab(), out=None) == EINVAL
    assert call(vocab(), tok=td.data_ptr() + 4) == EINVAL  # float4 loads need 16-byte alignment
    torch.cuda.synchronize()
    assert torch.all(desc == 7.0)  # nothing was launched
    assert call(vocab()) == 0
    torch.cuda.synchronize()
    want = _native.ops().vlad(td, cd)[0]
    assert torch.equal(desc, want)

    # k-means step and the whole forward: the same argument checks
    M = B * P
    nk = lib.mlg_kmeans_workspace_bytes(M, K)
    wk = torch.empty(nk, dtype=torch.uint8, device=dev)
    lab = torch.zeros(M, dtype=torch.int32, device=dev)
    chg = torch.zeros(1, dtype=torch.int64, device=dev)
    cnt = torch.zeros(K, dtype=torch.int32, device=dev)
    c2 = cd.clone()
    args = [td.data_ptr(), M, c2.data_ptr(), K, lab.data_ptr(), chg.data_ptr(), cnt.data_ptr(), wk.data_ptr(), nk, stream]
    for i, bad in ((0, None), (0, td.data_ptr() + 4), (1, 0), (2, None), (3, 24), (4, None), (5, None), (6, None),
                   (7, None), (8, nk - 1)):
        a = list(args)
        a[i] = bad
        assert lib.mlg_kmeans_step(*a) == EINVAL, i
    torch.cuda.synchronize()
    assert torch.equal(c2, cd)
    assert lib.mlg_anyloc_workspace_bytes(1, 518, 24) == 0 and lib.mlg_anyloc_workspace_bytes(1, 517, 64) == 0
    assert lib.mlg_anyloc_workspace_bytes(1, 518, 64) > lib.mlg_vit_workspace_bytes(1, 518)
    frames = torch.zeros(1, 32, 32, 3, dtype=torch.uint8, device=dev)
    v = vocab(struct_size=8)
    assert lib.mlg_anyloc_forward(None, ctypes.byref(v), frames.data_ptr(), 1, 32, 32, 3, 32 * 32 * 3, 518, 6,
                                  ws.data_ptr(), n, desc.data_ptr(), stream) == EINVAL


def test_malformed_weight_list_is_refused(dev, engine):
    """anyloc_forward checks every tensor of the ViT list before launching (weight_tables.h)."""
    from weight_corruptions import assert_refused
    x = torch.zeros(1, 32, 32, 3, dtype=torch.uint8, device=dev)
    vit = engine._vit
    assert_refused(lambda b: _native.ops().anyloc_forward(x, b, engine.centers, engine.image_size, vit.flags, 1),
                   vit._w, 0, "patch_w")
