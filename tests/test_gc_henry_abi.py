"""CPU: pcs_gc_henry (ABI 120) is declared, exported and bound with one signature, validates its arguments before it touches the
device, and its kernel fits the stack budget of tests/test_abi.py (the pattern of tests/test_gc_saturation_abi.py)."""
import ctypes
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["solute", "table", "S", "rows", "phi", "temp", "n", "h", "rho_vl", "p_sat", "dlnh_drho", "dpdrho_l", "status", "iters", "order",
         "stream"]


def test_header_symbol_and_binding_agree(hip_lib):
    from feos_torch_amd import GcPcSaftMix, _lib, native

    assert hip_lib.pcs_abi_version() >= 120  # 119 was pcs_pure_order_key
    assert hasattr(hip_lib, "pcs_gc_henry")
    with open(os.path.join(ROOT, "include", "pcsaft_hip.h")) as f:
        header = f.read()
    m = re.search(r"int pcs_gc_henry\(([^)]*)\);", header)
    assert m, "pcs_gc_henry is not declared in include/pcsaft_hip.h"
    declared = [" ".join(a.split()) for a in m.group(1).split(",")]
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    want = [ctypes.c_void_p if "*" in a else kinds[a.split()[0]] for a in declared]
    res, args = _lib.SIGNATURES["pcs_gc_henry"]
    assert res is ctypes.c_int and list(args) == want, (declared, args)
    assert [a.split()[-1].lstrip("*") for a in declared] == NAMES
    assert callable(native.gc_henry) and callable(GcPcSaftMix.henrys_law_constant)


def test_kernel_resources(hip_lib):
    from feos_torch_amd import build

    with open(build.RESOURCES) as f:
        res = json.load(f)
    assert "k_gc_henry" in res
    print("k_gc_henry:", res["k_gc_henry"], "k_gc_pure_vle:", res["k_gc_pure_vle"])
    assert res["k_gc_henry"]["scratch"] <= 2304, res["k_gc_henry"]
    assert "gc_henry.hip" in build.GUARDED_SOURCES  # the arithmetic of pcs_gc_pure_vle / pcs_gc_derivatives, IEEE NaN semantics
    assert hasattr(hip_lib, "pcs_gc_derivatives_vjp")  # the backward pass is made of an existing entry point


def test_argument_validation_without_gpu(hip_lib):
    L = hip_lib
    nul, one = None, ctypes.c_void_p(16)  # never dereferenced: the checks come first
    call = lambda solute, S, n, req, h, status, rows=None: L.pcs_gc_henry(solute, req, S, req if rows is None else rows, req, req, n, h,
                                                                          nul, nul, nul, nul, status, nul, nul, nul)
    assert call(0, 4, 0, nul, nul, nul) == 0 and call(1, 4, 0, one, one, one) == 0  # empty batch: returns at once
    assert call(0, 4, 5, one, one, nul) != 0  # status is required
    assert b"pcs_gc_henry" in L.pcs_last_error()
    assert call(0, 4, 5, one, nul, one) != 0  # h is required
    assert b"pcs_gc_henry" in L.pcs_last_error()
    assert call(0, 4, 5, nul, one, one) != 0  # and so are the inputs
    assert b"pcs_gc_henry" in L.pcs_last_error()
    for solute in (2, -1):
        assert call(solute, 4, 5, one, one, one) != 0
        assert b"solute" in L.pcs_last_error()
    assert call(1, 4, 5, one, one, one, rows=ctypes.c_void_p(8)) != 0
    assert b"16-byte aligned" in L.pcs_last_error()
    for S, n in ((4, -1), (4, 1 << 31), (0, 5), (33, 5)):
        assert call(0, S, n, one, one, one) != 0, (S, n)
        assert L.pcs_last_error() != b""
    assert call(0, 4, 0, nul, nul, nul) == 0 and L.pcs_last_error() == b""  # a clean call clears the message


def test_public_method_checks_the_solute_before_the_device():
    """The check stands in front of everything that needs a model or a device: an object without either raises it."""
    import numpy as np
    import pytest
    import torch

    from feos_torch_amd import GcPcSaftMix, native

    eos = GcPcSaftMix.__new__(GcPcSaftMix)  # no rows, no device: anything past the check would raise AttributeError
    T = torch.tensor([300.0], dtype=torch.float64)
    for solute in (2, -1, 0.5, 1.0, True, False, None, "0", np.float64(1.0)):
        with pytest.raises(ValueError, match="solute"):
            eos.henrys_law_constant(T, solute=solute)
    with pytest.raises(AttributeError):
        eos.henrys_law_constant(T)  # a valid solute goes on to the model
    with pytest.raises(ValueError, match="solute"):
        native.gc_henry(None, 4, None, None, T, solute=2)
    with pytest.raises(ValueError, match="solute"):
        native.gc_henry(None, 4, None, None, T, solute=True)
