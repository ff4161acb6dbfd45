"""CPU: the enthalpy-of-vaporization entry points exist in every layer (header, cross-compiled library, binding table, ABI
version, build recipe, compiler resource report) and the wrappers validate row counts on the host."""
import inspect
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"pcs_pure_enthalpy_of_vaporization": 7, "pcs_pure_enthalpy_of_vaporization_vjp": 8}


def test_header_library_and_bindings_carry_the_entry_points(hip_lib):
    from feos_torch_amd import _lib

    text = open(os.path.join(ROOT, "include", "pcsaft_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pcs_[a-z0-9_]+)\s*\(", text))
    for entry, nargs in ENTRIES.items():
        assert entry in declared, f"{entry} not declared in include/pcsaft_hip.h"
        assert hasattr(hip_lib, entry), f"{entry} not exported"
        assert entry in _lib.SIGNATURES and len(_lib.SIGNATURES[entry][1]) == nargs
    assert hip_lib.pcs_abi_version() >= 109


def test_resource_report_lists_the_new_kernels_within_their_budgets(hip_lib):
    """the per-lane stack limits of tests/test_abi.py: 2304 B, 3072 B for a kernel with vjp in its name"""
    from feos_torch_amd import build

    with open(build.RESOURCES) as f:
        res = json.load(f)
    assert "k_pure_enthalpy" in res and "k_pure_enthalpy_vjp" in res, sorted(res)
    assert res["k_pure_enthalpy"]["scratch"] <= 2304, res["k_pure_enthalpy"]
    assert res["k_pure_enthalpy_vjp"]["scratch"] <= 3072, res["k_pure_enthalpy_vjp"]


def test_unit_is_built_with_strict_ieee_flags():
    from feos_torch_amd import build

    units = [s for s in build.SOURCES if s[0] == "pure_enthalpy.hip"]
    assert len(units) == 1 and units[0][2] == []
    assert "pure_enthalpy.hip" not in build.RELAXED_SOURCES and "pure_enthalpy.hip" not in build.GUARDED_SOURCES


def test_argument_validation_without_gpu(hip_lib):
    import ctypes

    L = hip_lib
    nul = None
    one = ctypes.c_void_p(16)  # never dereferenced: the checks come first
    fwd = lambda n, req: L.pcs_pure_enthalpy_of_vaporization(req, req, n, nul, nul, req, nul)
    vjp = lambda n, req: L.pcs_pure_enthalpy_of_vaporization_vjp(req, req, req, n, req, nul, nul, nul)
    for call in (fwd, vjp):
        assert call(0, nul) == 0
        for n, req in ((-1, one), (1 << 31, one), (5, nul)):
            assert call(n, req) != 0, n
            assert L.pcs_last_error() != b"", n
        assert call(0, nul) == 0 and L.pcs_last_error() == b""  # a good call clears the message
    assert L.pcs_pure_enthalpy_of_vaporization(ctypes.c_void_p(8), one, 5, nul, nul, one, nul) != 0
    assert b"aligned" in L.pcs_last_error()
    assert L.pcs_pure_enthalpy_of_vaporization_vjp(ctypes.c_void_p(8), one, one, 5, one, nul, nul, nul) != 0
    assert b"aligned" in L.pcs_last_error()
    assert L.pcs_pure_enthalpy_of_vaporization_vjp(one, one, one, 5, one, ctypes.c_void_p(8), nul, nul) != 0
    assert b"aligned" in L.pcs_last_error()
    assert L.pcs_pure_enthalpy_of_vaporization_vjp(one, one, one, 5, nul, nul, nul, nul) != 0  # the cotangent is required
    assert b"null" in L.pcs_last_error()
    assert fwd(0, nul) == 0 and L.pcs_last_error() == b""  # leave no message behind for the tests that follow


def test_wrappers_refuse_differing_row_counts_before_any_launch(monkeypatch):
    """No GPU needed: _same_rows raises before the library is touched (the device lookup is the only thing stubbed)."""
    import torch

    from feos_torch_amd import native

    for fn in (native.pure_enthalpy_of_vaporization, native.pure_enthalpy_of_vaporization_vjp):
        src = inspect.getsource(fn)
        assert "_same_rows(" in src and "_call(" in src
    cpu = torch.device("cpu")
    monkeypatch.setattr(native, "_dev", lambda device=None: cpu)

    def no_library():
        raise AssertionError("the library was reached before the row counts were checked")

    monkeypatch.setattr(native._lib, "lib", no_library)
    f64 = torch.float64
    par, T, rho = torch.ones((4, 8), dtype=f64), torch.ones(4, dtype=f64), torch.ones((4, 2), dtype=f64)
    with pytest.raises(ValueError, match="temperature has 3 rows, expected 4"):
        native.pure_enthalpy_of_vaporization(par, T[:3])
    with pytest.raises(ValueError, match="temperature has 5 rows, expected 4"):
        native.pure_enthalpy_of_vaporization_vjp(par, torch.ones(5, dtype=f64), rho, T)
    with pytest.raises(ValueError, match="rho_vl has 3 rows, expected 4"):
        native.pure_enthalpy_of_vaporization_vjp(par, T, rho[:3], T)
    with pytest.raises(ValueError, match="gout has 2 rows, expected 4"):
        native.pure_enthalpy_of_vaporization_vjp(par, T, rho, T[:2])


def test_product_has_no_cpu_fallback_for_the_new_method():
    import torch

    if torch.cuda.is_available():
        return  # tests/test_enthalpy_gpu.py covers the method where it runs
    from feos_torch_amd import PcSaftPure, _lib

    eos = PcSaftPure(torch.tensor([[1.5, 3.5, 250.0, 0, 0.03, 1500.0, 1, 1]], dtype=torch.float64))
    with pytest.raises(_lib.PcsError):
        eos.enthalpy_of_vaporization(torch.tensor([300.0], dtype=torch.float64))
