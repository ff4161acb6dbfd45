"""CPU: the critical-point entry points exist in every layer (header, cross-compiled library, binding table, ABI version,
compiler resource report) and their wrappers validate row counts on the host."""
import inspect
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("pcs_pure_critical_point", "pcs_pure_critical_point_vjp")


def test_header_library_and_bindings_carry_both_entry_points(hip_lib):
    from feos_torch_amd import _lib

    text = open(os.path.join(ROOT, "include", "pcsaft_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pcs_[a-z0-9_]+)\s*\(", text))
    for s in ENTRY:
        assert s in declared, f"{s} not declared in include/pcsaft_hip.h"
        assert hasattr(hip_lib, s), f"{s} not exported"
        assert s in _lib.SIGNATURES
    assert hip_lib.pcs_abi_version() >= 106


def test_resource_report_lists_both_kernels_within_the_stack_budget(hip_lib):
    from feos_torch_amd import build

    with open(build.RESOURCES) as f:
        res = json.load(f)
    assert "k_pure_critical" in res and "k_pure_critical_vjp" in res, sorted(res)
    assert res["k_pure_critical"]["scratch"] <= 2304, res["k_pure_critical"]
    assert res["k_pure_critical_vjp"]["scratch"] <= 3072, res["k_pure_critical_vjp"]


def test_unit_is_built_with_strict_ieee_flags():
    from feos_torch_amd import build

    units = [s for s in build.SOURCES if s[0] == "pure_critical.hip"]
    assert len(units) == 1 and units[0][2] == []
    assert "pure_critical.hip" not in build.RELAXED_SOURCES and "pure_critical.hip" not in build.GUARDED_SOURCES


def test_argument_validation_without_gpu(hip_lib):
    import ctypes

    L = hip_lib
    nul = None
    one = ctypes.c_void_p(16)  # never dereferenced: the checks come first
    calls = {
        "pcs_pure_critical_point": lambda n, req: L.pcs_pure_critical_point(req, nul, n, nul, nul, nul, req, nul, nul),
        "pcs_pure_critical_point_vjp": lambda n, req: L.pcs_pure_critical_point_vjp(req, req, req, n, nul, nul, nul, req, nul),
    }
    for name, call in calls.items():
        assert call(0, nul) == 0, name
        for n, req in ((-1, one), (1 << 31, one), (5, nul)):
            assert call(n, req) != 0, (name, n)
            assert L.pcs_last_error() != b"", name
        assert call(0, nul) == 0 and L.pcs_last_error() == b""  # a good call clears the message


def test_wrappers_refuse_differing_row_counts_before_any_launch(monkeypatch):
    """No GPU needed: _same_rows raises before the library is touched (the device lookup is the only thing stubbed)."""
    import torch

    from feos_torch_amd import native

    for name in ("pure_critical_point", "pure_critical_point_vjp"):
        assert "_same_rows(" in inspect.getsource(getattr(native, name)), name
    cpu = torch.device("cpu")
    monkeypatch.setattr(native, "_dev", lambda device=None: cpu)

    def no_library():
        raise AssertionError("the library was reached before the row counts were checked")

    monkeypatch.setattr(native._lib, "lib", no_library)
    f64 = torch.float64
    par = torch.ones((4, 8), dtype=f64)
    with pytest.raises(ValueError, match="initial_temperature has 3 rows, expected 4"):
        native.pure_critical_point(par, torch.ones(3, dtype=f64))
    with pytest.raises(ValueError, match="parameters has 4 rows, expected 5"):
        native.pure_critical_point_vjp(par, torch.ones(5, dtype=f64), torch.ones(5, dtype=f64))
    with pytest.raises(ValueError, match="rho_c has 3 rows, expected 4"):
        native.pure_critical_point_vjp(par, torch.ones(4, dtype=f64), torch.ones(3, dtype=f64))
    with pytest.raises(ValueError, match="g_pc has 2 rows, expected 4"):
        native.pure_critical_point_vjp(par, torch.ones(4, dtype=f64), torch.ones(4, dtype=f64), g_pc=torch.ones(2, dtype=f64))
