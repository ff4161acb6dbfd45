"""Writes tests/golden/gc_jacobian_bits.json: per-row digests of the bits pcs_gc_jacobian returns (jac [n,7], agg [n,6]) for the
720-row batch of tests/test_gc_jacobian_bits_gpu.py, bubble and dew.  Run on the GPU at the commit whose behaviour is to be
pinned (ee50bd7 for the committed file: the last commit with k_gc_jacobian); inputs, calls and digests are those of the test
module.

    python tests/golden/make_golden_gc_jacobian_bits.py [out.json]

The recording is native.gc_jacobian without `order`, run twice; the two runs and every other call of the test module's CALLS
must give the same digests (asserted), so the file does not depend on which of them it was taken from."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gc_jacobian_bits_gpu as t  # noqa: E402

COMMIT = "ee50bd7"


def main(path):
    from feos_torch_amd import build, native
    from oracle import pyoracle

    build.build()
    build.build_host()
    pyoracle.build()
    out = {"commit": COMMIT, "n": t.gp.N}
    for dew in t.PROBLEMS:
        b = t.batch(pyoracle, dew)
        first = t.row_digests(*t.run(native, b, dew, t.CALLS[0]))
        for call in t.CALLS:
            assert t.row_digests(*t.run(native, b, dew, call)) == first, (t.name(dew), call)
        assert len(first) == t.gp.N
        out[t.name(dew)] = {"inputs": t.input_digest(b), "rows": "".join(first)}
        print(t.name(dew), "inputs", out[t.name(dew)]["inputs"], "rows", len(first), "distinct", len(set(first)))
    with open(path, "w") as f:
        f.write("{" + ",\n".join("%s:%s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in out.items()) + "}\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "gc_jacobian_bits.json"))
