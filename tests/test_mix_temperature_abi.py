"""CPU: the bubble / dew temperature entry point exists in every layer (header, cross-compiled library, binding table, ABI
version, build recipe, compiler resource report), validates its arguments without a device, and the wrappers validate row
counts on the host."""
import inspect
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "pcs_mix_bubble_dew_temperature"


def test_header_library_and_bindings_carry_the_entry_point(hip_lib):
    from feos_torch_amd import _lib

    text = open(os.path.join(ROOT, "include", "pcsaft_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pcs_[a-z0-9_]+)\s*\(", text))
    assert ENTRY in declared, f"{ENTRY} not declared in include/pcsaft_hip.h"
    assert hasattr(hip_lib, ENTRY), f"{ENTRY} not exported"
    assert ENTRY in _lib.SIGNATURES and len(_lib.SIGNATURES[ENTRY][1]) == 13
    assert hip_lib.pcs_abi_version() >= 110


def test_resource_report_lists_the_new_kernels_within_the_stack_limit(hip_lib):
    from feos_torch_amd import build

    with open(build.RESOURCES) as f:
        res = json.load(f)
    for name in ("void k_mix_temperature<false>", "void k_mix_temperature<true>"):
        assert name in res, sorted(res)
        assert res[name]["scratch"] <= 2304, (name, res[name])


def test_unit_is_built_guarded_like_the_bubble_dew_solver():
    from feos_torch_amd import build

    units = [s for s in build.SOURCES if s[0] == "mix_temperature.hip"]
    assert len(units) == 1 and units[0][2] == []
    assert "mix_temperature.hip" in build.GUARDED_SOURCES and "mix_temperature.hip" not in build.RELAXED_SOURCES


def test_argument_validation_without_gpu(hip_lib):
    import ctypes

    L = hip_lib
    nul = None
    one = ctypes.c_void_p(16)  # never dereferenced: the checks come first
    call = lambda n, req: L.pcs_mix_bubble_dew_temperature(0, req, req, req, req, req, n, nul, nul, req, nul, nul, nul)
    assert call(0, nul) == 0
    for n, req in ((-1, one), (1 << 31, one), (5, nul)):
        assert call(n, req) != 0, n
        assert L.pcs_last_error() != b"", n
    assert call(0, nul) == 0 and L.pcs_last_error() == b""  # a good call clears the message
    # each required pointer on its own
    for k in range(6):
        args = [one] * 6
        args[k] = nul
        assert L.pcs_mix_bubble_dew_temperature(1, *args[:5], 5, nul, nul, args[5], nul, nul, nul) != 0, k
        assert b"null required pointer" in L.pcs_last_error(), k
    odd = ctypes.c_void_p(8)
    assert L.pcs_mix_bubble_dew_temperature(0, odd, one, one, one, one, 5, nul, nul, one, nul, nul, nul) != 0
    assert b"aligned" in L.pcs_last_error()
    assert L.pcs_mix_bubble_dew_temperature(0, one, odd, one, one, one, 5, nul, nul, one, nul, nul, nul) != 0
    assert b"aligned" in L.pcs_last_error()
    assert L.pcs_mix_bubble_dew_temperature(0, one, one, one, one, one, 5, nul, odd, one, nul, nul, nul) != 0
    assert b"aligned" in L.pcs_last_error()
    assert call(0, nul) == 0 and L.pcs_last_error() == b""  # leave no message behind for the tests that follow


def test_wrapper_refuses_differing_row_counts_before_any_launch(monkeypatch):
    """No GPU needed: _same_rows raises before the library is touched (the device lookup is the only thing stubbed)."""
    import torch

    from feos_torch_amd import native

    assert "_same_rows(" in inspect.getsource(native.mix_bubble_dew_temperature)
    cpu = torch.device("cpu")
    monkeypatch.setattr(native, "_dev", lambda device=None: cpu)

    def no_library():
        raise AssertionError("the library was reached before the row counts were checked")

    monkeypatch.setattr(native._lib, "lib", no_library)
    f64 = torch.float64
    par, kij, v = torch.ones((4, 2, 8), dtype=f64), torch.zeros((4, 2), dtype=f64), torch.ones(4, dtype=f64)
    with pytest.raises(ValueError, match="kij has 3 rows, expected 4"):
        native.mix_bubble_dew_temperature(par, kij[:3], v, v, v, False)
    with pytest.raises(ValueError, match="pressure has 5 rows, expected 4"):
        native.mix_bubble_dew_temperature(par, kij, torch.ones(5, dtype=f64), v, v, False)
    with pytest.raises(ValueError, match="molefracs has 2 rows, expected 4"):
        native.mix_bubble_dew_temperature(par, kij, v, v[:2], v, True)
    with pytest.raises(ValueError, match="temperature has 3 rows, expected 4"):
        native.mix_bubble_dew_temperature(par, kij, v, v, v[:3], True)


def test_product_has_no_cpu_fallback_for_the_new_methods():
    import torch

    if torch.cuda.is_available():
        return  # tests/test_mix_temperature_gpu.py covers the methods where they run
    from feos_torch_amd import PcSaftMix, _lib

    f64 = torch.float64
    par = torch.tensor([[[1.5, 3.5, 250.0, 0, 0, 0, 0, 0], [2.5, 3.6, 260.0, 0, 0, 0, 0, 0]]], dtype=f64)
    v = lambda x: torch.tensor([x], dtype=f64)
    for name in ("bubble_temperature", "dew_temperature"):
        eos = PcSaftMix(par, torch.zeros((1, 2), dtype=f64))
        with pytest.raises(_lib.PcsError):
            getattr(eos, name)(v(1e5), v(0.5), v(300.0))
