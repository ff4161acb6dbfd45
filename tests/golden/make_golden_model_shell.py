"""Writes tests/golden/model_shell.json: the inputs of tests/test_model_shell_gpu.py and the bits every shell of the model
classes returns for them (values, gradients, Compaction, PureVlePlan).  Run on the GPU at the commit whose behaviour is to
be pinned (a55be04 for the committed file); the runners are those of the test module, which use the public API only.

    python tests/golden/make_golden_model_shell.py [out.json]

Everything is run twice.  A difference between the two runs is printed; for the gradients that are sums over the rows (gc
segment parameters, k_ab) the largest elementwise difference is stored as `spread` next to the first run's bits."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_model_shell_gpu as t  # noqa: E402


def grads_record(key, first, second):
    out = {}
    for name, g in first.items():
        if g is None:
            continue
        spread = float((g - second[name]).abs().max())
        if spread:
            print(f"two runs differ: {key} d/d{name} by {spread:.3e} (largest entry {float(g.abs().max()):.3e})")
            assert name in t.SUMMED, "only the sums over rows may depend on the run"
        out[name] = {"hex": t.to_hex(g), "spread": spread}
    return out


def tensors_record(key, first, second):
    for name in first:
        assert t.same_bits(first[name], second[name]), f"two runs differ: {key}/{name}"
    return {name: t.to_hex(v) for name, v in first.items()}


def main(path):
    import feos_torch_amd as amd
    from feos_torch_amd import native

    inputs = t.make_inputs()
    gold = {"commit": "a55be04", "inputs": inputs, "properties": {}, "derivatives": {}}
    for family, prop in t.CASES:
        for batch in ("a", "b"):
            inp = inputs[family] if batch == "a" else t.with_bad_row(inputs[family], family, prop)
            key = f"{t.prop_key(family, prop)}/{batch}"
            r1, r2 = (t.run_property(amd, family, prop, inp, "cuda", "all") for _ in range(2))
            for a, b in zip(r1["values"] + [r1["second"]], r2["values"] + [r2["second"]]):
                assert t.same_bits(a, b), f"two runs differ: {key}"
            assert r1["nans"].tolist() == [batch == "b" and i == t.BAD_ROW for i in range(t.N)], (key, r1["nans"])
            gold["properties"][key] = {"values": [t.to_hex(v) for v in r1["values"]], "second": t.to_hex(r1["second"]),
                                       "stable": None if r1["stable"] is None else r1["stable"].tolist(),
                                       "grads": grads_record(key, r1["grads"], r2["grads"])}
    for family in t.DERIV_FAMILIES:
        rec = {"grads": {}}
        for only in [None, 0, 1, 2] + ([] if family == "pure" else [3]):
            (o1, g1), (o2, g2) = (t.run_derivatives(amd, family, inputs[family], "cuda", only) for _ in range(2))
            assert all(t.same_bits(a, b) for a, b in zip(o1, o2)), f"two runs differ: derivatives/{family}"
            rec["outputs"] = [t.to_hex(o) for o in o1]
            name = "all" if only is None else f"only{only}"
            rec["grads"][name] = grads_record(f"derivatives/{family}/{name}", g1, g2)
        gold["derivatives"][family] = rec
    gold["compaction"] = tensors_record("compaction", t.run_compaction(native), t.run_compaction(native))
    bad = t.with_bad_row(inputs["pure"], "pure")
    gold["plan"] = tensors_record("plan", t.run_plan(native, bad), t.run_plan(native, bad))
    with open(path, "w") as f:
        json.dump(gold, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "model_shell.json"))
