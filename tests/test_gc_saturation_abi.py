"""CPU: pcs_gc_pure_vle (ABI 118) is declared, exported and bound with one signature, validates its arguments before it touches
the device, and its kernel fits the stack budget of tests/test_abi.py (the pattern of tests/test_henry_abi.py)."""
import ctypes
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["component", "table", "S", "rows", "phi", "temp", "n", "p_sat", "rho_vl", "dpdrho_vl", "status", "iters", "order", "stream"]


def test_header_symbol_and_binding_agree(hip_lib):
    from feos_torch_amd import GcPcSaftMix, _lib, native

    assert hip_lib.pcs_abi_version() >= 118  # 117 was pcs_mix_henry
    assert hasattr(hip_lib, "pcs_gc_pure_vle")
    with open(os.path.join(ROOT, "include", "pcsaft_hip.h")) as f:
        header = f.read()
    m = re.search(r"int pcs_gc_pure_vle\(([^)]*)\);", header)
    assert m, "pcs_gc_pure_vle is not declared in include/pcsaft_hip.h"
    declared = [" ".join(a.split()) for a in m.group(1).split(",")]
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    want = [ctypes.c_void_p if "*" in a else kinds[a.split()[0]] for a in declared]
    res, args = _lib.SIGNATURES["pcs_gc_pure_vle"]
    assert res is ctypes.c_int and list(args) == want, (declared, args)
    assert [a.split()[-1].lstrip("*") for a in declared] == NAMES
    assert callable(native.gc_pure_vle) and callable(GcPcSaftMix.vapor_pressure) and callable(GcPcSaftMix.equilibrium_liquid_density)


def test_kernel_resources(hip_lib):
    from feos_torch_amd import build

    with open(build.RESOURCES) as f:
        res = json.load(f)
    assert "k_gc_pure_vle" in res
    print("k_gc_pure_vle:", res["k_gc_pure_vle"])
    assert res["k_gc_pure_vle"]["scratch"] <= 2304, res["k_gc_pure_vle"]
    assert "gc_saturation.hip" in build.GUARDED_SOURCES  # the arithmetic of pcs_gc_derivatives, IEEE NaN / infinity semantics
    assert hasattr(hip_lib, "pcs_gc_derivatives_vjp")  # the backward pass is made of an existing entry point


def test_argument_validation_without_gpu(hip_lib):
    L = hip_lib
    nul, one = None, ctypes.c_void_p(16)  # never dereferenced: the checks come first
    call = lambda component, S, n, req, status, rows=None: L.pcs_gc_pure_vle(component, req, S, req if rows is None else rows, req, req,
                                                                             n, nul, nul, nul, status, nul, nul, nul)
    assert call(0, 4, 0, nul, nul) == 0 and call(1, 4, 0, one, one) == 0  # empty batch: returns at once
    assert call(0, 4, 5, one, nul) != 0  # status is required
    assert b"pcs_gc_pure_vle" in L.pcs_last_error()
    assert call(0, 4, 5, nul, one) != 0  # and so are the inputs
    assert b"pcs_gc_pure_vle" in L.pcs_last_error()
    for component in (2, -1):
        assert call(component, 4, 5, one, one) != 0
        assert b"component" in L.pcs_last_error()
    assert call(1, 4, 5, one, one, rows=ctypes.c_void_p(8)) != 0
    assert b"16-byte aligned" in L.pcs_last_error()
    for S, n in ((4, -1), (4, 1 << 31), (0, 5), (33, 5)):
        assert call(0, S, n, one, one) != 0, (S, n)
        assert L.pcs_last_error() != b""
    assert call(0, 4, 0, nul, nul) == 0 and L.pcs_last_error() == b""  # a clean call clears the message


def test_public_methods_check_the_component_before_the_device():
    """The check stands in front of everything that needs a model or a device: an object without either raises it."""
    import numpy as np
    import pytest
    import torch

    from feos_torch_amd import GcPcSaftMix, native

    eos = GcPcSaftMix.__new__(GcPcSaftMix)  # no rows, no device: anything past the check would raise AttributeError
    T = torch.tensor([300.0], dtype=torch.float64)
    for method in (eos.vapor_pressure, eos.equilibrium_liquid_density):
        for component in (2, -1, 0.5, 1.0, True, False, None, "0", np.float64(1.0)):
            with pytest.raises(ValueError, match="component"):
                method(T, component=component)
        with pytest.raises(AttributeError):
            method(T)  # a valid component goes on to the model
    with pytest.raises(ValueError, match="component"):
        native.gc_pure_vle(None, 4, None, None, T, component=2)
