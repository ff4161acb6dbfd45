"""CPU: the gc bubble / dew temperature entry point exists in every layer (header, cross-compiled library, binding table, ABI
version, build recipe, compiler resource report), validates its arguments without a device, and the wrapper validates row
counts on the host.  The mirror of tests/test_mix_temperature_abi.py."""
import inspect
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "pcs_gc_bubble_dew_temperature"


def test_header_library_and_bindings_carry_the_entry_point(hip_lib):
    from feos_torch_amd import _lib

    text = open(os.path.join(ROOT, "include", "pcsaft_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pcs_[a-z0-9_]+)\s*\(", text))
    assert ENTRY in declared, f"{ENTRY} not declared in include/pcsaft_hip.h"
    assert hasattr(hip_lib, ENTRY), f"{ENTRY} not exported"
    assert ENTRY in _lib.SIGNATURES and len(_lib.SIGNATURES[ENTRY][1]) == 15
    assert hip_lib.pcs_abi_version() >= 112


def test_resource_report_lists_the_new_kernels_within_the_stack_limit(hip_lib):
    from feos_torch_amd import build

    with open(build.RESOURCES) as f:
        res = json.load(f)
    for name in ("void k_gc_temperature<false>", "void k_gc_temperature<true>"):
        assert name in res, sorted(res)
        assert res[name]["scratch"] <= 2304, (name, res[name])


def test_unit_is_built_guarded_like_the_gc_bubble_dew_solver():
    from feos_torch_amd import build

    units = [s for s in build.SOURCES if s[0] == "gc_temperature.hip"]
    assert len(units) == 1 and units[0][2] == []
    assert "gc_temperature.hip" in build.GUARDED_SOURCES and "gc_temperature.hip" not in build.RELAXED_SOURCES
    assert "gc_kernels.hip" in build.GUARDED_SOURCES  # the unit whose cold solve it repeats


def test_argument_validation_without_gpu(hip_lib):
    import ctypes

    L = hip_lib
    nul = None
    one = ctypes.c_void_p(16)  # never dereferenced: the checks come first
    f = L.pcs_gc_bubble_dew_temperature
    # (dew, table, S, rows, phi, p_spec, z, t_init, n, t_out, rho4, status, iters, order, stream)
    call = lambda n, req, S=4: f(0, req, S, req, req, req, req, req, n, nul, nul, req, nul, nul, nul)
    assert call(0, nul) == 0
    for n, req in ((-1, one), (1 << 31, one), (5, nul)):
        assert call(n, req) != 0, n
        assert L.pcs_last_error() != b"", n
    assert call(0, nul) == 0 and L.pcs_last_error() == b""  # a good call clears the message
    for S in (0, 33):  # the table holds 1 to 32 segment types
        assert call(5, one, S) != 0, S
        assert b"segment types" in L.pcs_last_error(), S
    # each required pointer on its own: table, rows, phi, p_spec, z, t_init, status
    for k in range(7):
        a = [one] * 7
        a[k] = nul
        assert f(1, a[0], 4, a[1], a[2], a[3], a[4], a[5], 5, nul, nul, a[6], nul, nul, nul) != 0, k
        assert b"null required pointer" in L.pcs_last_error(), k
    odd = ctypes.c_void_p(8)
    assert f(0, one, 4, odd, one, one, one, one, 5, nul, nul, one, nul, nul, nul) != 0  # rows
    assert b"aligned" in L.pcs_last_error()
    assert f(0, one, 4, one, one, one, one, one, 5, nul, odd, one, nul, nul, nul) != 0  # rho4
    assert b"aligned" in L.pcs_last_error()
    assert call(0, nul) == 0 and L.pcs_last_error() == b""  # leave no message behind for the tests that follow


def test_wrapper_refuses_differing_row_counts_before_any_launch(monkeypatch):
    """No GPU needed: _check_gc and _same_rows raise before the library is touched."""
    import torch

    from feos_torch_amd import native

    src = inspect.getsource(native.gc_bubble_dew_temperature)
    assert "_check_gc(" in src and "_same_rows(" in src
    assert src.index("_check_gc(") < src.index("_call(") and src.index("_same_rows(") < src.index("_call(")

    def no_library():
        raise AssertionError("the library was reached before the row counts were checked")

    monkeypatch.setattr(native._lib, "lib", no_library)
    f64 = torch.float64
    S = 3
    table = torch.ones(S * 8 + 3 * S * S, dtype=f64)
    rows, phi, v = torch.zeros((4, 80), dtype=torch.uint8), torch.ones((4, 2), dtype=f64), torch.ones(4, dtype=f64)
    call = native.gc_bubble_dew_temperature
    with pytest.raises(ValueError, match="rows has 3 rows, expected 4"):
        call(table, S, rows[:3], phi, v, v, v, False)
    with pytest.raises(ValueError, match="phi has 5 rows, expected 4"):
        call(table, S, rows, torch.ones((5, 2), dtype=f64), v, v, v, False)
    with pytest.raises(ValueError, match="molefracs has 2 rows, expected 4"):
        call(table, S, rows, phi, v, v[:2], v, True)
    with pytest.raises(ValueError, match="temperature has 3 rows, expected 4"):
        call(table, S, rows, phi, v, v, v[:3], True)
    with pytest.raises(ValueError, match="table must be"):
        call(table[:-1], S, rows, phi, v, v, v, True)
    with pytest.raises(ValueError, match="order must be"):
        call(table, S, rows, phi, v, v, v, True, order=torch.zeros(3, dtype=torch.int32))


def test_product_has_no_cpu_fallback_for_the_new_methods():
    import torch

    if torch.cuda.is_available():
        return  # tests/test_gc_temperature_gpu.py covers the methods where they run
    from feos_torch_amd import _lib
    from feos_torch_amd.gc_pcsaft import _GcBubbleDew, GcPcSaftMix

    assert hasattr(GcPcSaftMix, "bubble_temperature") and hasattr(GcPcSaftMix, "dew_temperature")
    src = inspect.getsource(_GcBubbleDew)  # one Function serves the pressure and the temperature solve
    assert "native.gc_bubble_dew_temperature(" in src
    # a model cannot even be built without a device (the rows are encoded onto it): the constructor raises the library's error
    ident = ["A", "B"]
    par = [torch.ones(2, dtype=torch.float64) for _ in range(8)]
    with pytest.raises(_lib.PcsError):
        GcPcSaftMix(ident, par, [[["A", "B"], ["B"]]], [[[(0, 1)], []]], [])
