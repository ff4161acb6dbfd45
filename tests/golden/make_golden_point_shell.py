"""Writes tests/golden/point_shell.json: the inputs of tests/test_point_shell_gpu.py (taken from model_shell.json, which must
exist) and the bits, the masks and the C-ABI call lists the point properties return for them.  Run on the GPU at the commit
whose behaviour is to be pinned (f1a565d for the committed file); the runner is that of the test module, which uses the
public API only.

    python tests/golden/make_golden_point_shell.py [out.json]

Every pattern and backward pass is run twice.  The forward pass and every gradient that a pattern asks for must not depend
on the pattern (asserted), so they are stored once per case and backward pass, from the pattern "all".  A difference
between the two runs is printed; for the gradients that are sums over the rows (gc segment parameters, k_ab) the largest
elementwise difference is stored as `spread` next to the first run's bits.  One line per case."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_point_shell_gpu as t  # noqa: E402
from make_golden_model_shell import grads_record  # noqa: E402


def main(path):
    import feos_torch_amd as amd

    with open(os.path.join(HERE, "model_shell.json")) as f:
        inputs = t.make_inputs(json.load(f))
    cases = {}
    for case in t.CASES:
        for batch in ("a", "b"):
            inp = t.case_inputs(inputs, case, batch)
            key = f"{t.case_key(case)}/{batch}"
            rec = None
            for pattern in reversed(t.patterns(case)):  # "all" first
                for backward in t.backwards(case):
                    r1, r2 = (t.run_point(amd, case, inp, "cuda", pattern, backward) for _ in range(2))
                    # the condition of the pin: every row of batch a solves, row 2 alone is dropped in batch b
                    assert r1["nans"].tolist() == [batch == "b" and i == t.BAD_ROW for i in range(t.N)], (key, r1["nans"])
                    this = {"values": [t.pack(v) for v in r1["values"]], "nans": r1["nans"].tolist(),
                            "stable": None if r1["stable"] is None else r1["stable"].tolist(),
                            "second": [t.pack(v) for v in r1["second"]], "forward_calls": r1["forward_calls"]}
                    for a, b in zip(r1["values"] + r1["second"], r2["values"] + r2["second"]):
                        assert t.same_bits(a, b), f"two runs differ: {key}"
                    assert (r1["forward_calls"], r1["backward_calls"]) == (r2["forward_calls"], r2["backward_calls"]), key
                    if rec is None:
                        rec = dict(this, grads={}, backward_calls={})
                    assert this == {k: rec[k] for k in this}, f"{key}: the forward pass depends on what requires a gradient"
                    grads = {name: {"hex": "".join(g["hex"]), "spread": g["spread"]}
                             for name, g in grads_record(f"{key}/{pattern}/{backward}", r1["grads"], r2["grads"]).items()}
                    if pattern == "all":
                        rec["grads"][backward] = grads
                    for name, g in grads.items():
                        assert g == rec["grads"][backward][name], f"{key}: d/d{name} depends on the pattern {pattern}"
                    assert set(grads) == set(rec["grads"][backward]) & r1["required"], (key, pattern)
                    rec["backward_calls"][f"{pattern}/{backward}"] = r1["backward_calls"]
            cases[key] = rec
    dump = lambda obj: json.dumps(obj, separators=(",", ":"))
    with open(path, "w") as f:
        f.write('{"commit":"f1a565d",\n"inputs":%s,\n"cases":{\n%s\n}}\n'
                % (dump(inputs), ",\n".join(f"{dump(key)}:{dump(rec)}" for key, rec in cases.items())))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "point_shell.json"))
