"""CPU: pcs_pure_row_order and pcs_pure_vle_fast_ordered are declared, exported and bound with one signature, validate
their arguments before any launch, and k_pure_vle_ordered keeps the headline kernel's budget (no stack, four waves per SIMD)."""
import ctypes
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcs_pure_row_order", "pcs_pure_vle_fast_ordered")


def declared_parameters(name):
    """Parameter list of `name` in include/pcsaft_hip.h as 'p' (pointer) / 'i64' / 'int' per parameter."""
    text = open(os.path.join(ROOT, "include", "pcsaft_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} not declared"
    kinds = []
    for par in m.group(1).split(","):
        par = " ".join(par.split())
        kinds.append("p" if "*" in par else "i64" if par.startswith("int64_t") else "int")
    return kinds


def test_declared_exported_and_bound_with_one_signature(hip_lib):
    from feos_torch_amd import _lib

    kind_of = {ctypes.c_void_p: "p", ctypes.c_int64: "i64", ctypes.c_int: "int"}
    for name in NEW:
        assert hasattr(hip_lib, name), f"{name} not exported"
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int
        assert [kind_of[a] for a in args] == declared_parameters(name), name
    assert hip_lib.pcs_abi_version() >= 116


def test_arguments_are_validated_before_any_launch(hip_lib):
    L, nul, one = hip_lib, None, ctypes.c_void_p(8)  # `one` is never dereferenced: the checks come first
    calls = {
        "pcs_pure_row_order": lambda n, req: L.pcs_pure_row_order(req, req, n, req, nul),
        "pcs_pure_vle_fast_ordered": lambda n, req: L.pcs_pure_vle_fast_ordered(req, req, n, nul, nul, nul, req, nul, req, req, nul),
    }
    for name, call in calls.items():
        assert call(0, nul) == 0, name  # empty batch: nothing to check, nothing to do
        for n, req in ((-1, one), (1 << 31, one), (5, nul)):
            assert call(n, req) != 0, (name, n)
            assert L.pcs_last_error() != b"", name
    # each required pointer on its own
    for k in (0, 1, 3):
        a = [one, one, 5, one, nul]
        a[k] = nul
        assert L.pcs_pure_row_order(*a) != 0 and b"pcs_pure_row_order" in L.pcs_last_error(), k
    for k in (0, 1, 6, 8, 9):
        a = [one, one, 5, nul, nul, nul, one, nul, one, one, nul]
        a[k] = nul
        assert L.pcs_pure_vle_fast_ordered(*a) != 0 and b"pcs_pure_vle_fast_ordered" in L.pcs_last_error(), k
    # the pressure-only form only
    for k in (4, 5):
        a = [one, one, 5, nul, nul, nul, one, nul, one, one, nul]
        a[k] = one
        assert L.pcs_pure_vle_fast_ordered(*a) != 0 and b"pressure-only" in L.pcs_last_error(), k


def test_ordered_kernel_keeps_the_headline_budget(hip_lib):
    from feos_torch_amd import build

    with open(build.RESOURCES) as f:
        res = json.load(f)
    k = res["k_pure_vle_ordered"]
    assert k["scratch"] == 0 and k["occupancy"] >= 4, k
    assert k["lds"] == 256 * 9 * 8, k  # the staged rows (8 parameters + T, padded to 72 B) only: no perm, no bins
    assert res["k_pure_row_order"]["scratch"] == 0
    lite = [r for name, r in res.items() if "k_pure_vle<true, false>" in name]  # still exactly one headline kernel
    assert len(lite) == 1
