"""CPU: the boiling-temperature entry point and the Jacobian selector 3 exist in every layer (header, cross-compiled library,
binding table, ABI version, build recipe, compiler resource report) and the wrappers validate row counts on the host."""
import inspect
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "pcs_pure_boiling_temperature"


def test_header_library_and_bindings_carry_the_entry_point(hip_lib):
    from feos_torch_amd import _lib

    text = open(os.path.join(ROOT, "include", "pcsaft_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pcs_[a-z0-9_]+)\s*\(", text))
    assert ENTRY in declared, f"{ENTRY} not declared in include/pcsaft_hip.h"
    assert hasattr(hip_lib, ENTRY), f"{ENTRY} not exported"
    assert ENTRY in _lib.SIGNATURES and len(_lib.SIGNATURES[ENTRY][1]) == 9
    assert hip_lib.pcs_abi_version() >= 108


def test_resource_report_lists_the_new_kernels_within_their_budgets(hip_lib):
    """k_pure_boiling under the project's per-lane stack limit; the selector-3 Jacobian kernel (one kernel serves the plain
    and the vector-Jacobian form, like its siblings) within what tests/test_abi.py asks of selectors 0-2."""
    from feos_torch_amd import build

    with open(build.RESOURCES) as f:
        res = json.load(f)
    assert "k_pure_boiling" in res, sorted(res)
    assert res["k_pure_boiling"]["scratch"] <= 2304, res["k_pure_boiling"]
    jac = res["void k_pure_jacobian<3>"]
    assert jac["occupancy"] >= 2 and jac["scratch"] <= 256, jac


def test_unit_is_built_with_strict_ieee_flags():
    from feos_torch_amd import build

    units = [s for s in build.SOURCES if s[0] == "pure_boiling.hip"]
    assert len(units) == 1 and units[0][2] == []
    assert "pure_boiling.hip" not in build.RELAXED_SOURCES and "pure_boiling.hip" not in build.GUARDED_SOURCES


def test_argument_validation_without_gpu(hip_lib):
    import ctypes

    L = hip_lib
    nul = None
    one = ctypes.c_void_p(16)  # never dereferenced: the checks come first
    call = lambda n, req: L.pcs_pure_boiling_temperature(req, req, nul, n, nul, nul, req, nul, nul)
    assert call(0, nul) == 0
    for n, req in ((-1, one), (1 << 31, one), (5, nul)):
        assert call(n, req) != 0, n
        assert L.pcs_last_error() != b"", n
    assert call(0, nul) == 0 and L.pcs_last_error() == b""  # a good call clears the message
    assert L.pcs_pure_boiling_temperature(ctypes.c_void_p(8), one, nul, 5, nul, nul, one, nul, nul) != 0
    assert b"aligned" in L.pcs_last_error()
    assert L.pcs_pure_jacobian(7, one, one, nul, one, 5, one, nul) != 0  # unknown property selector
    assert b"which" in L.pcs_last_error()
    assert L.pcs_pure_jacobian_vjp(7, one, one, nul, one, one, 5, nul, nul, nul, nul) != 0
    assert b"which" in L.pcs_last_error()
    assert L.pcs_pure_jacobian(1, one, one, nul, one, 5, one, nul) != 0  # liquid_density still needs its pressure
    assert b"pressure" in L.pcs_last_error()
    assert call(0, nul) == 0 and L.pcs_last_error() == b""  # leave no message behind for the tests that follow


def test_selector_3_passes_validation_without_a_pressure(hip_lib):
    """Past the argument checks the call launches.  Without a device the launch itself is the only thing that can fail
    (return code 1 = HIP error; 2 = argument error); with one, real buffers are handed over and the call succeeds."""
    import ctypes

    import torch

    L = hip_lib
    nul = None
    if torch.cuda.is_available():
        f64 = torch.float64
        par = torch.tensor([[1.5, 3.5, 250.0, 0.0, 0.0, 0.0, 0.0, 0.0]] * 5, dtype=f64, device="cuda")
        T = torch.full((5,), 300.0, dtype=f64, device="cuda")
        rho = torch.tensor([[1e-4, 6e-3]] * 5, dtype=f64, device="cuda")
        jac = torch.empty((5, 10), dtype=f64, device="cuda")
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())
        assert L.pcs_pure_jacobian(3, ptr(par), ptr(T), nul, ptr(rho), 5, ptr(jac), nul) == 0, L.pcs_last_error()
        torch.cuda.synchronize()
        assert (jac[:, 8] == 0).all().item() and torch.isfinite(jac).all().item()
    else:
        one = ctypes.c_void_p(16)  # no device: nothing is launched, nothing dereferenced
        rc = L.pcs_pure_jacobian(3, one, one, nul, one, 5, one, nul)
        assert rc in (0, 1), L.pcs_last_error()
        assert b"which" not in L.pcs_last_error() and b"pressure" not in L.pcs_last_error()
        assert L.pcs_pure_jacobian(3, nul, nul, nul, nul, 0, nul, nul) == 0 and L.pcs_last_error() == b""  # message cleared


def test_wrappers_refuse_differing_row_counts_before_any_launch(monkeypatch):
    """No GPU needed: _same_rows raises before the library is touched (the device lookup is the only thing stubbed)."""
    import torch

    from feos_torch_amd import native

    assert "_same_rows(" in inspect.getsource(native.pure_boiling_temperature)
    cpu = torch.device("cpu")
    monkeypatch.setattr(native, "_dev", lambda device=None: cpu)

    def no_library():
        raise AssertionError("the library was reached before the row counts were checked")

    monkeypatch.setattr(native._lib, "lib", no_library)
    f64 = torch.float64
    par = torch.ones((4, 8), dtype=f64)
    with pytest.raises(ValueError, match="pressure has 3 rows, expected 4"):
        native.pure_boiling_temperature(par, torch.ones(3, dtype=f64))
    with pytest.raises(ValueError, match="initial_temperature has 5 rows, expected 4"):
        native.pure_boiling_temperature(par, torch.ones(4, dtype=f64), torch.ones(5, dtype=f64))
    rho = torch.ones((4, 2), dtype=f64)
    with pytest.raises(ValueError, match="parameters has 3 rows, expected 4"):
        native.pure_jacobian("boiling_temperature", par[:3], torch.ones(4, dtype=f64), None, rho)
    with pytest.raises(ValueError, match="gout has 2 rows, expected 4"):
        native.pure_jacobian_vjp("boiling_temperature", par, torch.ones(4, dtype=f64), None, rho, torch.ones(2, dtype=f64))
    assert native._WHICH["boiling_temperature"] == 3


def test_product_has_no_cpu_fallback_for_the_new_method():
    import torch

    if torch.cuda.is_available():
        return  # tests/test_boiling_gpu.py covers the method where it runs
    from feos_torch_amd import PcSaftPure, _lib

    eos = PcSaftPure(torch.tensor([[1.5, 3.5, 250.0, 0, 0.03, 1500.0, 1, 1]], dtype=torch.float64))
    with pytest.raises(_lib.PcsError):
        eos.boiling_temperature(torch.tensor([1e5], dtype=torch.float64))
