"""CPU: the C-ABI shared library loads and exports every symbol include/pcsaft_hip.h
declares; the Python binding table covers the header; and the product refuses to run
without a GPU instead of falling back to anything."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    text = open(os.path.join(ROOT, "include", "pcsaft_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pcs_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_entry_points():
    syms = header_symbols()
    assert "pcs_pure_vle" in syms and "pcs_last_error" in syms and len(syms) >= 7


def test_library_exports_every_declared_symbol(hip_lib):
    for s in header_symbols():
        assert hasattr(hip_lib, s), f"{s} declared in include/pcsaft_hip.h but not exported"


def test_binding_table_matches_header(hip_lib):
    from feos_torch_amd import _lib

    assert sorted(_lib.SIGNATURES) == header_symbols()


def test_abi_version_and_error_string(hip_lib):
    assert hip_lib.pcs_abi_version() >= 100
    assert hip_lib.pcs_last_error() == b""
    assert hip_lib.pcs_workspace_bytes(1000) == 4 * (1000 + 64)  # row order / retry list + control block
    assert hip_lib.pcs_mix_workspace_bytes(1000) == 4 * (1000 + 64) + (32 + 32 + 4) * 1000  # + fugacities and densities, init records, robust list


def test_argument_validation_without_gpu(hip_lib):
    """Every entry point rejects bad sizes / missing required pointers before it touches the device: non-zero return,
    message in pcs_last_error, and n = 0 is a no-op (the reference panics on invalid input, src/pcsaft.rs:89)."""
    import ctypes

    L = hip_lib
    nul = None
    one = ctypes.c_void_p(8)  # never dereferenced: the checks come first
    calls = {
        "pcs_pure_vle": lambda n, req: L.pcs_pure_vle(req, req, n, nul, nul, nul, req, nul, req, nul),
        "pcs_pure_vapor_pressure": lambda n, req: L.pcs_pure_vapor_pressure(req, req, n, nul, nul, req, req, nul),
        "pcs_compact_rows": lambda n, req: L.pcs_compact_rows(req, n, req, req, 8, req, nul, nul),
        "pcs_expand_rows": lambda n, req: L.pcs_expand_rows(req, n, req, nul, req, 10, 0, 8, req, nul),
        "pcs_pure_liquid_density": lambda n, req: L.pcs_pure_liquid_density(req, req, req, n, nul, nul, req, nul),
        "pcs_pure_derivatives": lambda n, req: L.pcs_pure_derivatives(req, req, req, n, nul, nul, nul, nul),
        "pcs_mix_bubble_dew": lambda n, req: L.pcs_mix_bubble_dew(0, req, req, req, req, req, n, nul, nul, req, nul, nul, nul),
        "pcs_mix_derivatives": lambda n, req: L.pcs_mix_derivatives(req, req, req, req, n, nul, nul, nul, nul, nul),
        "pcs_mix_jacobian": lambda n, req: L.pcs_mix_jacobian(0, req, req, req, req, n, req, nul, nul),
        "pcs_gc_bubble_dew": lambda n, req: L.pcs_gc_bubble_dew(0, req, 4, req, req, req, req, req, n, nul, nul, req, nul, nul, nul, nul),
    }
    for name, call in calls.items():
        assert call(0, nul) == 0, name  # empty batch: nothing to check, nothing to do
        for n, req in ((-1, one), (1 << 31, one), (5, nul)):
            assert call(n, req) != 0, (name, n)
            assert L.pcs_last_error() != b"", name
    assert L.pcs_compact_plan(nul, 5, one, nul) != 0 and L.pcs_compact_plan(one, 5, nul, nul) != 0
    assert L.pcs_compact_rows(one, 5, one, one, 0, one, nul, nul) != 0 and b"width" in L.pcs_last_error()
    assert L.pcs_expand_rows(one, 5, one, nul, one, 10, 4, 8, one, nul) != 0 and b"column" in L.pcs_last_error()
    assert L.pcs_compact_workspace_bytes(10_000_000) == 4 * (2 + 4883 + 2)
    assert L.pcs_pure_jacobian(7, one, one, nul, one, 5, one, nul) != 0  # unknown property selector
    assert b"which" in L.pcs_last_error()


def test_product_has_no_cpu_fallback():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from feos_torch_amd import PcSaftPure, _lib

    eos = PcSaftPure(torch.tensor([[1.5, 3.5, 250.0, 0, 0.03, 1500.0, 1, 1]], dtype=torch.float64))
    with pytest.raises(_lib.PcsError):
        eos.vapor_pressure(torch.tensor([300.0], dtype=torch.float64))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "feos_torch_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "pyoracle" not in src and "liboracle" not in src and "from oracle" not in src, f


def test_kernel_stack_frames_and_occupancy(hip_lib):
    """Compiler report of the last build (feos_torch_amd/build/resources.json).  Large per-lane stack frames make the
    runtime throttle the resident waves (the mixture Jacobian ran at 21 ms instead of 10 ms per 1e6 rows with a
    2.5-4 KB frame), so every kernel is held below 2.25 KB; the headline kernel must keep its
    four waves per SIMD (122 VGPRs; the SLP vectoriser alone costs it one of them) and use no stack at all; the pure
    Jacobian kernels must keep two."""
    import json

    from feos_torch_amd import build

    with open(build.RESOURCES) as f:
        res = json.load(f)
    assert len(res) >= 20
    for name, r in res.items():
        # the T2<DN> probes of the state-function VJP kernels (backward of `derivatives`, not on any benchmark path)
        # need a larger frame; they are held below 3 KB
        limit = 3072 if ("vjp" in name or "k_gc_segment_gradient<1," in name or "k_mixn" in name) else 2304
        if "k_mixn_derivatives_vjp" in name:
            # the backward pass of the n-component state functions is correct-first: one DN<1> forward-mode pass per input
            # direction through the fully inlined model, 4-25 KB of stack per lane for 1-6 components (not on any benchmark path)
            limit = 26 * 1024
        assert r["scratch"] <= limit, (name, r)
    lite = [r for name, r in res.items() if "k_pure_vle<true, false>" in name]
    assert len(lite) == 1 and lite[0]["scratch"] == 0 and lite[0]["occupancy"] >= 4, lite
    polish = [r for name, r in res.items() if "k_pure_vle<true, true>" in name]  # + the exact Newton update of the densities
    assert len(polish) == 1 and polish[0]["scratch"] <= 192 and polish[0]["occupancy"] >= 4, polish
    rho = res["k_pure_vle_rho"]  # the pressure-only kernel handing out polished densities (pcs_pure_vapor_pressure)
    assert rho["scratch"] <= 192 and rho["occupancy"] >= 4, rho
    for which in range(3):
        jac = res[f"void k_pure_jacobian<{which}>"]
        assert jac["occupancy"] >= 2 and jac["scratch"] <= 256, (which, jac)
    # the all-fp64 VLE kernel and the liquid-density kernel trade a small spill frame for one / two more resident waves
    # (measured faster, csrc/pure_kernels.hip); the others use no stack
    full = res["void k_pure_vle<false, false>"]
    assert full["occupancy"] >= 4 and full["scratch"] <= 320, full
    k2 = res["k_pure_liquid_density"]
    assert k2["occupancy"] >= 3 and k2["scratch"] <= 160, k2
    for name in ("k_pure_vle_fallback", "k_pure_vle_robust", "k_pure_derivatives"):
        assert res[name]["scratch"] == 0, (name, res[name])


def test_row_count_validation_is_host_side():
    """The kernels launch one lane per temperature over every row-wise argument, so the wrappers must refuse any
    argument with another number of rows before launching (the reference raises a shape error there; easy to hit: every
    property call reduces the model, so a later `derivatives(T, rho)` with the original T is one row too long)."""
    import torch

    from feos_torch_amd import native

    f64 = torch.float64
    native._same_rows(4, parameters=torch.zeros((4, 8), dtype=f64), density=torch.zeros(4, dtype=f64), pressure=None)
    with pytest.raises(ValueError, match="parameters has 3 rows, expected 4"):
        native._same_rows(4, parameters=torch.zeros((3, 8), dtype=f64), density=torch.zeros(4, dtype=f64))
    with pytest.raises(ValueError, match="rho4 has 5 rows"):
        native._same_rows(4, rho4=torch.zeros((5, 4), dtype=f64))
    S = 3
    table = torch.zeros(S * 8 + 3 * S * S, dtype=f64)
    rows = torch.zeros((4, 80), dtype=torch.uint8)
    native._check_gc(table, S, rows, 4)
    with pytest.raises(ValueError, match="rows has 4 rows, expected 5"):
        native._check_gc(table, S, rows, 5)
    with pytest.raises(ValueError, match="table must be"):
        native._check_gc(table[:-1], S, rows, 4)
    with pytest.raises(ValueError, match="rows must be"):
        native._check_gc(table, S, rows[:, :79], 4)
    # every device-level wrapper validates (source check: a new wrapper without a row check is the bug this guards)
    import inspect

    for name in ("pure_vle", "pure_liquid_density", "pure_derivatives", "pure_jacobian", "mix_bubble_dew", "mix_derivatives",
                 "mix_jacobian", "gc_bubble_dew", "gc_derivatives", "gc_jacobian"):
        src = inspect.getsource(getattr(native, name))
        assert "_same_rows(" in src or "differ in length" in src, name
