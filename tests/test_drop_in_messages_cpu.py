"""Every drop-in class of mlgate.vpr / mlgate.verify down each of its branches, without a GPU:
the engine constructors (and the two resolvers vpr.py calls itself) are replaced by stubs that
record their arguments, and the ordered warnings, the stub calls, the exception and the flags
each branch leaves behind are compared with tests/golden/drop_in_messages.json, recorded by
tests/golden/make_drop_in_messages.py before the native-branch switch was written once.

A branch is {cls, kw (constructor), set (attributes set afterwards, e.g. native), env (the
MLGATE_* variables; all others are cleared), sources ({stub: weights_source}, default
'synthetic(seed=0)'), do (what is called)}."""
import contextlib
import importlib
import inspect
import json
import os
import warnings
from unittest import mock

import numpy as np
import pytest
import torch

from mlgate import verify, vpr
from mlgate import weights as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "drop_in_messages.json")
IMG = np.zeros((32, 32, 3), np.uint8)
ENGINES = {"ResNet50GPU": "resnet", "MixVprGPU": "mixvpr", "SaladGPU": "salad", "AnyLocGPU": "anyloc",
           "CricaGPU": "crica", "engine_for": "vit", "SuperPointGPU": "superpoint", "LightGlueGPU": "lightglue",
           "SuperGlueGPU": "superglue", "LoFTRGPU": "loftr", "OrbGPU": "orb"}
RESOLVERS = ("resolve_state_dict", "resolve_crica_state_dict")
FLAGS = ("_model_loaded", "_is_fallback", "_is_native", "feat_dim")
HELD = ("_net", "_mix", "_salad", "_vit", "_anyloc", "_crica", "extractor", "matcher", "_matcher", "_fallback", "orb")


def _show(v):
    if isinstance(v, dict):
        return f"<dict of {len(v)}>"
    if isinstance(v, np.ndarray):
        return f"<array {v.shape} {v.dtype}>"
    return repr(v)


def _log(calls, name, real, a, kw):
    """Record a stub call as the arguments the real callable would have bound (defaults filled
    in, **kwargs flattened): how a value was passed is not behaviour, a call the real signature
    refuses is a TypeError here too."""
    sig = inspect.signature(real)
    bound = sig.bind(*a, **kw)
    bound.apply_defaults()
    args = {}
    for k, v in bound.arguments.items():
        args.update(v if sig.parameters[k].kind is inspect.Parameter.VAR_KEYWORD else {k: v})
    calls.append([name, {k: _show(v) for k, v in sorted(args.items())}])


def _engine(name, real, calls, sources):
    class Engine:
        device = "stub-device"

        def __init__(self, *a, **kw):
            _log(calls, name, real, a, kw)
            self.weights_source = sources.get(name, "synthetic(seed=0)")
            self.group = kw.get("group", 1)

        def forward(self, frames, with_local=False):
            return (torch.zeros(1, 4), torch.zeros(1, 2, 4)) if with_local else torch.zeros(1, 4)

        def forward_device(self, frames, dim):
            return torch.zeros(1, dim)

    Engine.__name__ = Engine.__qualname__ = name
    return Engine


def _resolver(name, real, calls, sources):
    def resolve(*a, **kw):
        _log(calls, name, real, a, kw)
        return {"stub": 0}, sources.get(name, "synthetic(seed=0)")
    return resolve


def run(branch):
    """{'warnings': [[category, text]], 'calls': [[stub, {argument: value}]], 'error': [type, text] | None,
    'flags': {...}, 'held': {attribute: class name}} of one branch."""
    calls, sources = [], branch.get("sources", {})
    env = {k: v for k, v in os.environ.items() if not k.startswith("MLGATE_")}
    env.update(branch.get("env", {}))
    with contextlib.ExitStack() as stack:
        stack.enter_context(mock.patch.dict(os.environ, env, clear=True))
        for name, module in ENGINES.items():
            mod = importlib.import_module("mlgate." + module)
            stack.enter_context(mock.patch.object(mod, name, _engine(name, getattr(mod, name), calls, sources)))
        for name in RESOLVERS:
            stack.enter_context(mock.patch.object(W, name, _resolver(name, getattr(W, name), calls, sources)))
        stack.enter_context(mock.patch.object(vpr, "_device_frames", lambda images, device: "frames"))
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            obj = branch["cls"](**branch.get("kw", {}))
            for k, v in branch.get("set", {}).items():
                setattr(obj, k, v)
            error = None
            try:
                branch["do"](obj)
            except Exception as e:  # noqa: BLE001  (the type is part of what is recorded)
                error = [type(e).__name__, str(e)]
    return {"warnings": [[w.category.__name__, str(w.message)] for w in caught], "calls": calls, "error": error,
            "flags": {a: _show(getattr(obj, a)) for a in FLAGS if hasattr(obj, a)},
            "held": {a: type(getattr(obj, a)).__name__ for a in HELD if hasattr(obj, a)}}


def _describe(m):
    m.extract_descriptor(IMG)


def _describe_twice_regrouped(m):
    m.extract_descriptor(IMG)
    m.cross_image_group = 3
    m.extract_descriptors([IMG])


def _add(m):
    m.add_image(IMG, 1.0, floor_label=2, image_path="a.png")
    m.add_images([IMG], [2.0])


def _load(m):
    m._load_model()


def _vpr(cls, native_var, wrong, engine, extra=()):
    """The branches every VPR class has; ``wrong`` = {name: constructor kwargs the native branch refuses}."""
    on = {"set": {"native": True}}
    out = {"default": {}, "native_true": on, "env": {"env": {native_var: "1"}},
           "env_other_value": {"env": {native_var: "true"}},
           "native_false_env": {"set": {"native": False}, "env": {native_var: "1"}},
           "native_configured": dict(on, sources={engine: "/w/model.ckpt", "resolve_state_dict": "/w/dino.pth",
                                                  "resolve_crica_state_dict": "/w/crica.pth"}),
           "default_configured": {"sources": {"ResNet50GPU": "/w/rn50.pth", "resolve_state_dict": "/w/dino.pth"}}}
    out.update({name: dict(on, kw=kw) for name, kw in wrong.items()})
    out.update(extra)
    return {f"{cls.__name__}.{k}": dict(v, cls=cls, do=v.get("do", _describe)) for k, v in out.items()}


def _matcher(cls, branches):
    return {f"{cls.__name__}.{k}": dict(v, cls=cls, do=_load) for k, v in branches.items()}


BRANCHES = {
    **_vpr(vpr.MixVPR, "MLGATE_MIXVPR_NATIVE", {"wrong_dim": {"descriptor_dim": 512},
                                               "wrong_backbone": {"backbone": "resnet18"}}, "MixVprGPU",
           {"native_path": {"set": {"native": True}, "kw": {"pretrained_path": "/w/mix.ckpt", "device": "cuda:1"}},
            "default_other_dim": {"kw": {"descriptor_dim": 512, "backbone": "resnet18"}}}),
    **_vpr(vpr.SALAD, "MLGATE_SALAD_NATIVE", {"wrong_dim": {"descriptor_dim": 4096}}, "SaladGPU",
           {"native_path": {"set": {"native": True}, "kw": {"pretrained_path": "/w/salad.ckpt"}}}),
    **_vpr(vpr.AnyLoc, "MLGATE_ANYLOC_NATIVE", {"wrong_dim": {"descriptor_dim": 1000},
                                               "wrong_clusters": {"num_clusters": 60, "descriptor_dim": 60 * 768},
                                               "wrong_backbone": {"backbone": "dinov2_vits14"},
                                               "fewer_clusters": {"num_clusters": 32, "descriptor_dim": 32 * 768}},
           "AnyLocGPU",
           {"default_vits": {"kw": {"backbone": "dinov2_vits14"}},
            "default_unknown_backbone": {"kw": {"backbone": "dinov2_vitg14"}},
            "native_batch": {"set": {"native": True}, "do": lambda m: m.extract_descriptors([IMG])}}),
    **_vpr(vpr.CricaVPR, "MLGATE_CRICAVPR_NATIVE", {"wrong_dim": {"descriptor_dim": 768},
                                                   "wrong_backbone": {"backbone": "dinov2_vitl14"}}, "CricaGPU",
           {"native_path": {"set": {"native": True}, "kw": {"pretrained_path": "/w/crica.pth"}},
            "default_vitl_path": {"kw": {"backbone": "dinov2_vitl14", "pretrained_path": "/w/l.pth"}},
            "default_unknown_backbone": {"kw": {"backbone": "resnet50"}},
            "native_group_2": {"set": {"native": True, "cross_image_group": 2}},
            "native_group_80": {"set": {"native": True, "cross_image_group": 80}},
            "native_regrouped": {"set": {"native": True}, "do": _describe_twice_regrouped},
            "native_add": {"set": {"native": True}, "do": _add},
            "default_add": {"do": _add}}),
    **_matcher(verify.LightGlue, {
        "default": {}, "kw": {"kw": {"device": "cuda:1", "max_keypoints": 512, "detection_threshold": 0.01}},
        "fallback_1": {"env": {"MLGATE_LIGHTGLUE_FALLBACK": "1"}},
        "fallback_orb": {"env": {"MLGATE_LIGHTGLUE_FALLBACK": "ORB"}, "kw": {"max_keypoints": 500}},
        "fallback_other_value": {"env": {"MLGATE_LIGHTGLUE_FALLBACK": "0"}},
        "superpoint_configured": {"sources": {"SuperPointGPU": "/w/sp.pth"}},
        "lightglue_configured": {"sources": {"LightGlueGPU": "/w/lg.pth"}},
        "both_configured": {"sources": {"SuperPointGPU": "/w/sp.pth", "LightGlueGPU": "/w/lg.pth"}}}),
    **_matcher(verify.SuperGlue, {
        "default": {}, "native_true": {"set": {"native": True}, "kw": {"max_keypoints": 1024}},
        "env": {"env": {"MLGATE_SUPERGLUE_NATIVE": "1"}},
        "native_false_env": {"set": {"native": False}, "env": {"MLGATE_SUPERGLUE_NATIVE": "1"}},
        "superpoint_configured": {"set": {"native": True}, "sources": {"SuperPointGPU": "/w/sp.pth"}},
        "superglue_configured": {"set": {"native": True}, "sources": {"SuperGlueGPU": "/w/sg.pth"}},
        "both_configured": {"set": {"native": True},
                            "sources": {"SuperPointGPU": "/w/sp.pth", "SuperGlueGPU": "/w/sg.pth"}}}),
    **_matcher(verify.LoFTR, {
        "default": {}, "native_true": {"set": {"native": True}}, "env": {"env": {"MLGATE_LOFTR_NATIVE": "1"}},
        "env_checkpoint": {"env": {"MLGATE_LOFTR_WEIGHTS": "/w/loftr.ckpt"}, "sources": {"LoFTRGPU": "/w/loftr.ckpt"}},
        "native_false_env": {"set": {"native": False},
                             "env": {"MLGATE_LOFTR_NATIVE": "1", "MLGATE_LOFTR_WEIGHTS": "/w/loftr.ckpt"}},
        "outdoor_without_checkpoint": {"set": {"native": True}, "kw": {"weights": "outdoor"}},
        "outdoor_env_without_checkpoint": {"env": {"MLGATE_LOFTR_NATIVE": "1"}, "kw": {"weights": "outdoor"}},
        "outdoor_with_checkpoint": {"kw": {"weights": "outdoor", "device": "cuda:1"},
                                    "env": {"MLGATE_LOFTR_WEIGHTS": "/w/out.ckpt"},
                                    "sources": {"LoFTRGPU": "/w/out.ckpt"}}}),
}


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_recorded_branch_is_still_driven():
    assert sorted(golden()) == sorted(BRANCHES)


@pytest.mark.parametrize("name", BRANCHES)
def test_branch(name):
    got = json.loads(json.dumps(run(BRANCHES[name])))  # tuples as the lists JSON holds
    want = golden()[name]
    for part in ("error", "warnings", "calls", "flags", "held"):
        assert got[part] == want[part], part
