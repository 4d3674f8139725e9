"""Fixtures that pin what the Python layer says and constructs, for refactors of it:

  * drop_in_messages.json -- per branch of every drop-in class (tests/test_drop_in_messages_cpu.py
    BRANCHES): the ordered warnings, the engine constructor arguments, the exception, the flags;
  * checkpoint_messages.json -- per model of mlgate.weights (tests/test_checkpoints_cpu.py): the
    KeyError of a file that lacks three keys, the three source strings of the resolver, and the
    model-specific refusals.

The recording code is the tests' own (their ``run`` / ``record_*``), so what is written is
what they compare.  Run it on the commit whose behaviour is to be kept; no GPU is needed.

    python tests/golden/make_drop_in_messages.py      # ~20 s
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "multi-level-indoor-slam_amd"), os.path.join(ROOT, "tests")]


def write(name, obj):
    with open(os.path.join(HERE, name), "w") as f:
        json.dump(obj, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    import test_checkpoints_cpu as C
    import test_drop_in_messages_cpu as D
    write("drop_in_messages.json", {name: D.run(b) for name, b in D.BRANCHES.items()})
    with tempfile.TemporaryDirectory() as tmp:
        out = {model: C.record_model(model, tmp) for model in C.MODELS}
        out["refusals"] = C.record_refusals(tmp)
    write("checkpoint_messages.json", out)


if __name__ == "__main__":
    main()
