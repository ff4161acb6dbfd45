#!/usr/bin/env python3
"""scripts/dev/isa_span.py <unit.s> [kernel substring]: static VALU counts of the head, the solver body and the epilogue of
k_pure_vle_ordered in a device-only assembly file (hipcc ... --cuda-device-only -S with build.py's flags for pure_kernels.hip,
or the file isa_diff.py --keep leaves).  The solver is inlined, so the spans are cut by what only it does:
  head      entry .. the first v_cvt_f32_f64 (pure_coef_f32 narrowing the staged row: the first instruction of the solve);
  epilogue  the last label before the first global store / atomic .. s_endpgm (the live test, result stores, list append);
  body      what lies between.
Per span: VALU in all, 64-bit integer VALU (shifts, adds, compares, multiply-adds on register pairs), v_cndmask, v_cmp,
v_mov, and the vector memory / LDS / barrier instructions.  The head is straight-line code: its static count is what every
wave executes.  Also the kernel's register, LDS and scratch figures from its descriptor."""
import re
import sys

INT64 = re.compile(r"v_(lshl_add_u64|lshlrev_b64|lshrrev_b64|ashrrev_i64|mad_[iu]64_[iu]32|cmpx?_\w+_[iu]64|add_co_u32|addc_co_u32|sub_co_u32|subb_co_u32)")


def kernel_lines(path, key):
    out, on = [], False
    for raw in open(path):
        s = raw.split(";")[0].strip()
        if re.match(r"^_Z\w*%s\w*:" % key, s):
            on = True
            continue
        if on and s.startswith(".Lfunc_end"):
            break
        if on and s:
            out.append(s)
    return out


def count(lines):
    c = {"valu": 0, "int64": 0, "cndmask": 0, "cmp": 0, "mov": 0, "vmem": 0, "lds": 0, "barrier": 0, "salu": 0}
    for s in lines:
        op = s.split()[0]
        if op.startswith("v_"):
            c["valu"] += 1
            c["int64"] += bool(INT64.match(op))
            c["cndmask"] += op.startswith("v_cndmask")
            c["cmp"] += op.startswith("v_cmp")
            c["mov"] += op.startswith("v_mov")
        elif op.startswith(("global_", "flat_", "buffer_")):
            c["vmem"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op == "s_barrier":
            c["barrier"] += 1
        elif op.startswith("s_") and not op.startswith(("s_waitcnt", "s_nop")):
            c["salu"] += 1
    return c


def main():
    path, key = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "k_pure_vle_ordered")
    lines = kernel_lines(path, key)
    code = [s for s in lines if not s.startswith(".") or s.endswith(":")]
    first_solve = next(k for k, s in enumerate(code) if s.startswith("v_cvt_f32_f64"))
    first_store = next(k for k, s in enumerate(code) if s.startswith(("global_store", "global_atomic")))
    epi = max(k for k, s in enumerate(code[:first_store]) if s.endswith(":"))
    for name, span in (("head", code[:first_solve]), ("body", code[first_solve:epi]), ("epilogue", code[epi:])):
        c = count(span)
        print(f"{name:9s} " + "  ".join(f"{k} {v}" for k, v in c.items()))
    for s in lines:
        m = re.match(r"\.amdhsa_(group_segment_fixed_size|private_segment_fixed_size|next_free_vgpr|next_free_sgpr)\s+(\d+)", s)
        if m:
            print(f"{m.group(1)} {m.group(2)}")


if __name__ == "__main__":
    main()
