#!/usr/bin/env python3
"""scripts/dev/isa_diff.py <tree A> <tree B> [--keep DIR]: is the device code of two checkouts the same?

Compiles every translation unit of feos_torch_amd/build.py's SOURCES in both trees with that tree's own flags for the
unit + --cuda-device-only -S (as isa_count.sh does) and prints, per device function, whether the instruction text and
the kernel descriptor are identical.  A plain text comparison: the __hip_cuid_* lines, .file, .ident and comment lines
are dropped, and local labels lose the ordinal of their function within the unit (.LBB<k>_<n> -> .LBB_<n>: a function
removed from or added to a unit renumbers all that follow it); nothing else is interpreted.  Exit status 1 if any function
differs or exists in one tree only.
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def unit_commands(tree, out_dir):
    """[(label, command)]: one device-only assembly run per (source, object) pair of the tree's build.py"""
    path = os.path.join(tree, "feos_torch_amd", "build.py")
    spec = importlib.util.spec_from_file_location("_build_" + str(abs(hash(path))), path)
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    cmds = []
    for entry in b.SOURCES:
        src, obj, extra = entry[:3]
        if hasattr(b, "unit_flags"):
            flags = b.unit_flags(entry)
        else:  # a tree from before unit_flags: its build() composed the flags like this
            flags = (b.FLAGS + (b.RELAXED if src in b.RELAXED_SOURCES else []) + (b.REASSOC if "-DPCS_PURE_PART=1" in extra else [])
                     + (b.GUARDED if src in b.GUARDED_SOURCES else []) + extra)
        label = obj[:-2]
        cmds.append((label, ["hipcc"] + flags + ["--cuda-device-only", "-S", "-o", os.path.join(out_dir, label + ".s"),
                             os.path.join(b.CSRC, src)]))
    return cmds


def functions(path):
    """{symbol: (is_kernel, [instruction lines], [descriptor lines])} of one assembly file"""
    out, cur, desc = {}, None, None
    for raw in open(path):
        s = raw.split(";")[0].strip()  # comments, at the start of a line or behind an instruction, carry no code
        if not s or s.startswith("//") or "__hip_cuid_" in s or s.startswith(".file") or s.startswith(".ident"):
            continue
        s = re.sub(r"\.L(BB|JTI)\d+_", r".L\1_", s)
        m = re.match(r"^\.type\s+(\S+),@function", s)
        if m:
            cur = out.setdefault(m.group(1), [False, [], []])
        elif s.startswith(".Lfunc_end"):
            cur = None
        elif s.startswith(".amdhsa_kernel "):
            desc = out.setdefault(s.split()[1], [False, [], []])
            desc[0] = True
        elif s == ".end_amdhsa_kernel":
            desc = None
        elif desc is not None:
            desc[2].append(s)
        elif cur is not None:
            cur[1].append(s)
    return {k: v for k, v in out.items() if v[1]}


def demangle(names):
    try:
        res = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
        return {n: d.replace("(anonymous namespace)::", "").split("(")[0] for n, d in zip(names, res)}
    except Exception:
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--keep", help="directory for the .s files (default: a temporary one)")
    ap.add_argument("--jobs", type=int, default=min(10, os.cpu_count() or 1))
    a = ap.parse_args()
    top = a.keep or tempfile.mkdtemp(prefix="isa_diff_")
    dirs = []
    for side, tree in (("a", a.tree_a), ("b", a.tree_b)):
        d = os.path.join(top, side)
        os.makedirs(d, exist_ok=True)
        dirs.append(d)
    cmds = unit_commands(a.tree_a, dirs[0]) + unit_commands(a.tree_b, dirs[1])
    with ThreadPoolExecutor(a.jobs) as ex:
        for (label, cmd), r in zip(cmds, ex.map(lambda c: subprocess.run(c[1], capture_output=True, text=True), cmds)):
            if r.returncode != 0:
                sys.exit(f"{label}: hipcc failed\n{r.stderr}")
    labels = sorted({label + ".s" for label, _ in cmds})
    differ = 0
    for f in labels:
        pa, pb = os.path.join(dirs[0], f), os.path.join(dirs[1], f)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"{f[:-2]}: unit exists in one tree only")
            differ += 1
            continue
        fa, fb = functions(pa), functions(pb)
        names = demangle(sorted(set(fa) | set(fb)))
        for sym in sorted(set(fa) | set(fb)):
            kind = "kernel  " if (fa.get(sym) or fb.get(sym))[0] else "function"
            if sym not in fa or sym not in fb:
                verdict = "ONLY IN " + ("A" if sym in fa else "B")
            elif fa[sym][1] == fb[sym][1] and fa[sym][2] == fb[sym][2]:
                verdict = "identical"
            else:
                verdict = f"DIFFERENT ({len(fa[sym][1])} -> {len(fb[sym][1])} lines)"
            differ += verdict != "identical"
            print(f"{f[:-2]:18s} {kind} {verdict:32s} {names[sym]}")
    print(f"{differ} device function(s) differ" if differ else "all device functions identical")
    if not a.keep:
        print(f"(assembly left in {top})")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
