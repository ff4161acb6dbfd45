"""Writes tests/golden/bd_driver_bits.json: inputs and recorded bits of tests/test_bd_driver_bits_gpu.py.  Run on the GPU with
the library of the commit whose behaviour is to be pinned (88307fe for the committed file: build that checkout's
libpcsaft_hip.so and select it with PCS_HIP_LIB); rows, calls and records are those of the test module.

    PCS_HIP_LIB=<88307fe>/feos_torch_amd/libpcsaft_hip.so python tests/golden/make_golden_bd_driver_bits.py [out.json] [--robust FILE]

--robust FILE: JSON {"bubble": [...], "dew": [...]}, the rows of mix_batch(200_000, seed=78) that only the robust second
attempt solves (status of pcs_mix_bubble_dew 0 with the library, 1 with a build of the same commit in which BdLane::start
ends a robust lane at once); the first ROBUST_KEEP per problem are kept.  Without it the indices of the existing file are
reused, with the rows that follow the first ROBUST_KEEP of the dew list (rows whose restarted attempt needs most of its
evaluation budget, see the test module).  p_spec of the temperature cases and rho4 of the Jacobian cases are the library's own bubble / dew points at the batch
temperature (1e5 Pa and RHO4_UNSOLVED on rows it does not solve).  Every case is run twice and must give the same record."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_bd_driver_bits_gpu as t  # noqa: E402

COMMIT = "88307fe"


def main(path, robust_file):
    import torch
    from feos_torch_amd import build, native

    build.build_host()
    if robust_file:
        with open(robust_file) as f:
            robust = {k: sorted(v)[:t.ROBUST_KEEP] for k, v in json.load(f).items()}
    else:
        with open(path) as f:
            robust = json.load(f)["robust"]
    out = {"commit": COMMIT, "robust": robust, "inputs": {}, "cases": {}}
    for dew in t.PROBLEMS:
        inp = {}
        out["inputs"][t.name(dew)] = {}
        for batch in ("mix", "gc", "robust"):
            if batch == "gc":
                rows, const = t.gc_rows()
                p, rho4, status, _ = t.gc_bubble_dew(native, rows, const, dew, True)
            else:
                rows = t.mix_rows(t.N, t.MIX_SEED) if batch == "mix" else t.mix_rows(t.ROBUST_N, t.ROBUST_SEED, robust[t.name(dew)])
                const = {}
                p, rho4, status, _ = t.mix_bubble_dew(native, rows, const, dew, True)
            ok = status == 0
            rows["p_spec"] = torch.where(ok, p, torch.full_like(p, t.P_UNSOLVED))
            g = {"p_spec": t.hex_of(rows["p_spec"])}
            if batch != "gc":
                rows["rho4"] = torch.where(ok[:, None], rho4, torch.tensor(t.RHO4_UNSOLVED, dtype=t.f64, device=rho4.device)).contiguous()
                g["rho4"] = t.hex_of(rows["rho4"])
            inp[batch] = (rows, const)
            out["inputs"][t.name(dew)][batch] = g
            print(t.name(dew), batch, "rows", int(ok.numel()), "solved", int(ok.sum()))
        cases = {}
        for case, run in t.CASES.items():
            rows, const = inp[case.split("/")[0]]
            first, second = (t.strip(run(native, rows, const, dew)) for _ in range(2))
            assert first == second, f"two runs differ: {t.name(dew)}, {case}"
            cases[case] = first
            print(t.name(dew), case, "failed rows", first.get("status", "").count("1"))
        out["cases"][t.name(dew)] = cases
    dump = lambda obj: json.dumps(obj, separators=(",", ":"))
    with open(path, "w") as f:
        f.write('{"commit":%s,\n"robust":%s,\n"inputs":%s,\n"cases":{\n%s\n}}\n' % (
            dump(COMMIT), dump(robust), dump(out["inputs"]),
            ",\n".join("%s:{\n%s\n}" % (dump(k), ",\n".join(f"{dump(c)}:{dump(r)}" for c, r in v.items())) for k, v in out["cases"].items())))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    args = sys.argv[1:]
    robust_file = None
    if "--robust" in args:
        k = args.index("--robust")
        robust_file = args[k + 1]
        del args[k:k + 2]
    main(args[0] if args else os.path.join(HERE, "bd_driver_bits.json"), robust_file)
