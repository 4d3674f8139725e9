"""The checkpoint loaders and resolvers of mlgate.weights, model by model, without a GPU:
every accepted file layout gives back the keys of ``*_keys()`` in order, as float32, with the
bits that were written; a file that lacks keys, a resolver's three sources and the
model-specific refusals say exactly what tests/golden/checkpoint_messages.json records
(tests/golden/make_drop_in_messages.py wrote it from the loaders as they were before they
were folded into one table).

SALAD and CricaVPR carry a ViT-B trunk (about 340 MB of float32), so each is written at full
size once, in its most wrapped layout; every other file of those two, and every file of the
error and precedence tests, is "thin": each tensor stores one element broadcast to its shape,
which keeps the keys, shapes and dtypes a loader looks at and a value it must pass through."""
import functools
import json
import os
import re
from unittest import mock

import numpy as np
import pytest
import torch

from mlgate import weights as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "checkpoint_messages.json")
VITS = "dinov2_vits14"


def _old_lightglue(sd):
    """The key names of older LightGlue releases: 'matcher.' in front, self_attn.{i}.* / cross_attn.{i}.*."""
    return {"matcher." + re.sub(r"^transformers\.(\d+)\.(self_attn|cross_attn)\.", r"\2.\1.", k): v
            for k, v in sd.items()}


def _prefixed(prefix):
    return lambda sd: {prefix + k: v for k, v in sd.items()}


def _under(*names):
    def wrap(sd):
        for n in reversed(names):
            sd = {n: sd}
        return sd
    return wrap


# model -> (load, resolve(path, seed), keys, synthetic(seed), environment variable, {layout: wrap})
MODELS = {
    "dinov2": (lambda p: W.load_hub_state_dict(p, VITS), lambda p, s: W.resolve_state_dict(p, s, VITS),
               lambda: W.hub_keys(VITS), lambda s: W.synthetic_state_dict(s, VITS), "MLGATE_DINOV2_WEIGHTS",
               {"bare": dict, "model": _under("model")}),
    "superpoint": (W.load_superpoint_state_dict, W.resolve_superpoint_state_dict,
                   lambda: [f"{n}.{p}" for n, *_ in W.SUPERPOINT_LAYERS for p in ("weight", "bias")],
                   W.superpoint_state_dict, "MLGATE_SUPERPOINT_WEIGHTS", {"bare": dict}),
    "lightglue": (W.load_lightglue_state_dict, W.resolve_lightglue_state_dict, W.lightglue_keys,
                  W.lightglue_state_dict, "MLGATE_LIGHTGLUE_WEIGHTS", {"bare": dict, "old": _old_lightglue}),
    "resnet50": (W.load_resnet50_state_dict, W.resolve_resnet50_state_dict, W.resnet50_keys, W.resnet50_state_dict,
                 "MLGATE_RESNET50_WEIGHTS", {"bare": dict}),
    "loftr": (W.load_loftr_state_dict, W.resolve_loftr_state_dict, W.loftr_keys, W.loftr_state_dict,
              "MLGATE_LOFTR_WEIGHTS", {"bare": dict, "state_dict": _under("state_dict")}),
    "superglue": (W.load_superglue_state_dict, W.resolve_superglue_state_dict, W.superglue_keys,
                  W.superglue_state_dict, "MLGATE_SUPERGLUE_WEIGHTS", {"bare": dict}),
    "salad": (W.load_salad_state_dict, W.resolve_salad_state_dict, W.salad_keys, W.salad_state_dict,
              "MLGATE_SALAD_WEIGHTS", {"state_dict": _under("state_dict"), "bare": dict}),
    "mixvpr": (W.load_mixvpr_state_dict, W.resolve_mixvpr_state_dict, W.mixvpr_keys, W.mixvpr_state_dict,
               "MLGATE_MIXVPR_WEIGHTS", {"bare": dict, "state_dict": _under("state_dict")}),
    "crica": (W.load_crica_state_dict, W.resolve_crica_state_dict, W.crica_keys, W.crica_state_dict,
              "MLGATE_CRICAVPR_WEIGHTS",
              {"model_state_dict+module": lambda sd: _under("model_state_dict")(_prefixed("module.")(sd)),
               "bare": dict, "state_dict": _under("state_dict"), "module": _prefixed("module."),
               "model_state_dict": _under("model_state_dict")}),
}
BIG = ("salad", "crica")  # full size in their first layout only


@functools.lru_cache(maxsize=None)
def synthetic(model, seed=0):
    """The seeded weights of ``model``: computed once, shared, never written to."""
    return MODELS[model][3](seed)


def thin(sd, shift=0.0):
    """{key: tensor of sd[key]'s shape and dtype holding one stored element (its first, + shift)}."""
    out = {}
    for k, v in sd.items():
        v = np.asarray(v)
        one = torch.from_numpy(v.reshape(-1)[:1] + v.dtype.type(shift))
        out[k] = one.expand(v.shape) if v.ndim else one.reshape(())
    return out


def full(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def save(obj, tmp, name):
    path = os.path.join(str(tmp), name)
    torch.save(obj, path)
    return path


def _text(exc, *paths):
    s = exc.args[0] if isinstance(exc, KeyError) else str(exc)
    for i, p in enumerate(paths):
        s = s.replace(p, "{path%d}" % i)
    return [type(exc).__name__, s]


def _raised(fn, *paths):
    try:
        fn()
    except Exception as e:  # noqa: BLE001  (the type is part of what is recorded)
        return _text(e, *paths)
    return None


# ------------------------------------------------------------------ what the fixture records
def record_model(model, tmp):
    """{'missing': [type, text], 'sources': [...]} of one model, paths replaced by {path0}, {path1}."""
    load, resolve, keys, _, env, _ = MODELS[model]
    sd = synthetic(model)
    ks = keys()
    gone = (ks[1], ks[len(ks) // 2], ks[-1])
    lacking = save({k: v for k, v in thin(sd).items() if k not in gone}, tmp, f"{model}_lacking.pth")
    a, b = save(thin(sd), tmp, f"{model}_a.pth"), save(thin(sd, 1.0), tmp, f"{model}_b.pth")
    first = lambda got: float(np.asarray(got[ks[0]]).reshape(-1)[0])  # noqa: E731
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MLGATE_")}
    sources, values = [], []
    for arg, var in ((a, b), (None, b), (None, None)):
        with mock.patch.dict(os.environ, dict(clean, **({env: var} if var else {})), clear=True):
            got, source = resolve(arg, 3)
        assert list(got) == ks if (arg or var) else sorted(got) == sorted(ks)  # seeded: the generator's order
        sources.append(source.replace(a, "{path0}").replace(b, "{path1}"))
        values.append(first(got))
    want = first(sd)
    assert values[0] == want and values[1] == np.float32(want + 1)  # the argument's file, then the variable's
    return {"missing": _raised(lambda: load(lacking), lacking), "sources": sources}


def record_refusals(tmp):
    out = {}
    for have, ask in (("dinov2_vitb14", "dinov2_vitl14"), (VITS, "dinov2_vitb14")):
        shapes = W.hub_shapes(have)
        path = save({k: torch.zeros(1).expand(shapes[k]) for k in W.hub_keys(have)}, tmp, f"{have}.pth")
        out[f"{have} asked for as {ask}"] = _raised(lambda: W.load_hub_state_dict(path, ask), path)
    sd = thin(synthetic("crica"))
    path = save(dict(sd, **{"backbone.blocks.0.adapter.weight": torch.zeros(4, 4)}), tmp, "adapter.pth")
    out["crica with an adapter"] = _raised(lambda: W.load_crica_state_dict(path), path)
    path = save(dict(sd, **{"aggregation.1.p": torch.full((2,), 3.0)}), tmp, "head.pth")
    out["crica head of the wrong size"] = _raised(lambda: W.load_crica_state_dict(path), path)
    return out


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ------------------------------------------------------------------ the tests
@pytest.mark.parametrize("model", MODELS)
def test_valid_file_in_each_layout(model, tmp_path):
    load, _, keys, _, _, layouts = MODELS[model]
    sd = synthetic(model)
    assert sorted(sd) == sorted(keys())
    for i, (layout, wrap) in enumerate(layouts.items()):
        slim = model in BIG and i > 0
        path = save(wrap(thin(sd) if slim else full(sd)), tmp_path, f"{model}_{i}.pth")
        got = load(path)
        os.remove(path)
        assert list(got) == keys(), layout
        for k, v in got.items():
            want = np.asarray(sd[k])
            if slim:
                want = np.broadcast_to(want.reshape(-1)[0], want.shape)
            assert v.dtype == np.float32 and v.shape == want.shape, (layout, k)
            assert np.array_equal(v, want), (layout, k)


@pytest.mark.parametrize("model", MODELS)
def test_missing_keys_and_resolver_precedence(model, tmp_path):
    """A file without three keys raises the recorded KeyError; resolve_* takes the argument
    before the environment variable before seeded weights and names each source as recorded."""
    got, want = record_model(model, tmp_path), golden()[model]
    assert got["missing"] == want["missing"] and got["missing"][0] == "KeyError"
    assert got["sources"] == want["sources"] == ["{path0}", "{path1}", "synthetic(seed=3)"]


def test_synthetic_source_is_the_seeded_network():
    for model in MODELS:
        if model in BIG:
            continue  # record_model has checked their keys; the values are the generators' own tests
        got, _ = MODELS[model][1](None, 3)
        want = synthetic(model, 3)
        assert all(np.array_equal(got[k], want[k]) and got[k].dtype == np.float32 for k in MODELS[model][2]())


def test_model_specific_refusals(tmp_path):
    got, want = record_refusals(tmp_path), golden()["refusals"]
    assert got == want
    assert [v[0] for v in got.values()] == ["ValueError"] * 4


def test_crica_head_of_another_shape_but_the_right_size_is_reshaped(tmp_path):
    sd = thin(synthetic("crica"))
    path = save(dict(sd, **{"aggregation.1.p": torch.tensor(3.0)}), tmp_path, "scalar_p.pth")
    got = W.load_crica_state_dict(path)
    assert got["aggregation.1.p"].shape == (1,) and got["aggregation.1.p"][0] == 3.0
