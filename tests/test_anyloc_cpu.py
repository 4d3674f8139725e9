"""AnyLoc's native branch without a GPU: properties of the float64 restatement
(tests/anyloc_restatement.py), the vocabulary loaders, the drop-in's argument errors, and
the conditions the GPU tests' fixtures must meet (asserted here so tests/test_anyloc_gpu.py
can rely on them)."""
import numpy as np
import pytest
import torch

import anyloc_restatement as R
from mlgate.vpr import AnyLoc
from mlgate.weights import load_vocabulary, synthetic_vocabulary


# ------------------------------------------------------------------ restatement
def test_descriptor_is_a_unit_vector_with_unit_blocks():
    tokens, centers = R.head_fixture((2, 65, 64))
    labels = R.assign(tokens[1], centers)[0]
    v = R.vlad(tokens[1], centers)
    assert v.shape == (64 * 768,) and abs(np.linalg.norm(v) - 1) < 1e-12
    blocks = np.linalg.norm(v.reshape(64, 768), axis=1)
    used = np.bincount(labels, minlength=64) > 0
    assert 0 < used.sum() < 64
    assert np.all(blocks[~used] == 0)  # an empty cluster: a zero block
    assert np.allclose(blocks[used], 1 / np.sqrt(used.sum()), rtol=1e-12)  # intra-normalised, then one global norm


def test_single_token():
    tokens, centers = R.head_fixture((1, 1, 16))
    lab, gap, second = R.assign(tokens[0], centers)
    v = R.vlad(tokens[0], centers).reshape(16, 768)
    want = R.unit(R.unit(tokens[0, 0]) - centers[lab[0]].astype(np.float64))
    assert np.allclose(v[lab[0]], want, rtol=0, atol=1e-15)
    assert np.count_nonzero(np.linalg.norm(v, axis=1)) == 1 and second[0] != lab[0] and gap[0] > 0


def test_zero_token_gets_label_zero_and_ties_go_to_the_lowest_cluster():
    tokens, centers = R.head_fixture((2, 65, 64))
    assert not tokens[0, 1].any()
    lab, gap, _ = R.assign(tokens[0], centers)
    assert lab[1] == 0 and gap[1] == 0
    twice = np.concatenate([centers[5:6], centers])  # centre 5 now also at 0
    t = centers[5:6] * 3.0
    assert R.assign(t, twice)[0][0] == 0
    # its residual is -c_0: the block is not skipped
    v = R.vlad(tokens[0, 1:2], centers).reshape(64, 768)
    assert np.allclose(v[0], -R.unit(centers[0]), atol=1e-12)


def test_f32_variant_is_the_same_function():
    tokens, centers = R.head_fixture((2, 65, 64))
    lab = R.assign(tokens[1], centers)[0]
    e = R.one_minus_cos(R.vlad_f32(tokens[1], centers, lab), R.vlad(tokens[1], centers, lab))
    assert 0 < e < 1e-13  # float32 rounding only (amplitude ~1e-7, squared)


# ------------------------------------------------------------------ vocabulary files
def test_vocabulary_round_trip(tmp_path):
    c = synthetic_vocabulary(32, seed=4)
    assert c.shape == (32, 768) and c.dtype == np.float32
    np.save(tmp_path / "v.npy", c)
    torch.save(torch.from_numpy(c), tmp_path / "bare.pt")
    torch.save({"c_centers": torch.from_numpy(c).double()}, tmp_path / "c_centers.pt")
    for name in ("v.npy", "bare.pt", "c_centers.pt"):
        got = load_vocabulary(tmp_path / name)
        assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, c), name
    assert np.array_equal(load_vocabulary(str(tmp_path / "v.npy"), 32), c)


@pytest.mark.parametrize("shape", [(64, 767), (24, 768), (144, 768), (768,), (2, 16, 768)])
def test_vocabulary_wrong_shape(tmp_path, shape):
    np.save(tmp_path / "bad.npy", np.zeros(shape, np.float32))
    torch.save(torch.zeros(shape), tmp_path / "bad.pt")
    torch.save({"c_centers": torch.zeros(shape)}, tmp_path / "bad_dict.pt")
    for name in ("bad.npy", "bad.pt", "bad_dict.pt"):
        with pytest.raises(ValueError):
            load_vocabulary(tmp_path / name)


def test_vocabulary_other_errors(tmp_path):
    np.save(tmp_path / "v.npy", synthetic_vocabulary(32))
    with pytest.raises(ValueError):
        load_vocabulary(tmp_path / "v.npy", 64)  # not the K asked for
    torch.save({"centers": torch.zeros(64, 768)}, tmp_path / "nokey.pt")
    with pytest.raises(ValueError):
        load_vocabulary(tmp_path / "nokey.pt")


# ------------------------------------------------------------------ drop-in errors
@pytest.mark.parametrize("kw, names", [({"descriptor_dim": 768}, ("768", "64")), ({"num_clusters": 24}, ("24", "49152")),
                                       ({"num_clusters": 32}, ("32", "49152"))])
def test_native_rejects_inconsistent_dimensions(kw, names, monkeypatch):
    monkeypatch.delenv("MLGATE_ANYLOC_NATIVE", raising=False)
    m = AnyLoc(**kw)
    m.native = True
    img = np.zeros((32, 32, 3), np.uint8)
    for call in (lambda: m.extract_descriptor(img), lambda: m.extract_descriptors([img])):
        with pytest.raises(ValueError) as e:
            call()
        assert all(n in str(e.value) for n in names), str(e.value)
    monkeypatch.setenv("MLGATE_ANYLOC_NATIVE", "1")
    env = AnyLoc(**kw)
    assert env.native is None
    with pytest.raises(ValueError):
        env.extract_descriptor(img)


def test_set_vocabulary_checks_the_shape():
    m = AnyLoc()
    with pytest.raises(ValueError):
        m.set_vocabulary(np.zeros((32, 768), np.float32))  # num_clusters is 64
    with pytest.raises(ValueError):
        m.set_vocabulary(np.zeros((64, 512), np.float32))
    m.set_vocabulary(synthetic_vocabulary(64))


# ------------------------------------------------------------------ fixture conditions
@pytest.mark.parametrize("shape", R.HEAD_SHAPES)
def test_head_fixture_has_few_undecided_tokens(shape):
    tokens, centers = R.head_fixture(shape)
    norms = np.linalg.norm(centers, axis=1)
    assert np.all(np.abs(norms - 0.87) < 0.1)
    under = 0
    for b in range(shape[0]):
        under += int(np.sum(R.assign(tokens[b], centers)[1] < R.GAP_DECIDED))
    print(shape, "tokens under the margin:", under)
    # the zero token is always undecided; beyond it at most 0.5 % of the tokens
    assert under - (1 if shape[1] > 1 else 0) <= R.UNDECIDED_CAP * shape[0] * shape[1]
    if shape == (3, 63, 128):
        assert all(len(set(R.assign(tokens[b], centers)[0])) < 128 for b in range(3))  # empty clusters


def test_planted_mixture_is_decided_at_every_step():
    x = R.planted_mixture()
    assert x.shape == (2000, 768)
    centers, labels, n_iter, min_gap = R.kmeans(x, 16, R.KMEANS_SEED)
    print("steps", n_iter, "minimum gap", min_gap)
    assert min_gap >= R.KMEANS_MIN_GAP
    assert n_iter == 3 and len(set(labels)) == 16
    floor = np.abs(R.kmeans_update_f32(x, labels, centers) - centers).max()
    assert 0 < floor < 1e-6


def test_e2e_fixture_has_few_undecided_tokens():
    f = R.e2e_fixture()
    n = int(f["F"].sum())
    print("tokens under 1e-4:", n, "minimum gap", f["gap"].min(), "e_flip", f["e_flip"], "e_f32", f["e_f32"])
    assert f["tokens"].shape == (3, 1368, 768)
    assert n <= R.E2E_F_CAP * 1368
    assert f["e_f32"] < 1e-12  # no block that is rounding noise alone (a one-token cluster at its own centre)
