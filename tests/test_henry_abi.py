"""CPU: pcs_mix_henry (ABI 117) is declared, exported and bound with one signature, validates its arguments before it touches
the device, and its kernel fits the stack budget of tests/test_abi.py."""
import ctypes
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbol_and_binding_agree(hip_lib):
    from feos_torch_amd import PcSaftMix, _lib, native

    assert hip_lib.pcs_abi_version() >= 117  # 116 was taken by the pure row order before this entry point was added
    assert hasattr(hip_lib, "pcs_mix_henry")
    with open(os.path.join(ROOT, "include", "pcsaft_hip.h")) as f:
        header = f.read()
    m = re.search(r"int pcs_mix_henry\(([^)]*)\);", header)
    assert m, "pcs_mix_henry is not declared in include/pcsaft_hip.h"
    declared = [" ".join(a.split()) for a in m.group(1).split(",")]
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    want = [ctypes.c_void_p if "*" in a else kinds[a.split()[0]] for a in declared]
    res, args = _lib.SIGNATURES["pcs_mix_henry"]
    assert res is ctypes.c_int and list(args) == want, (declared, args)
    assert [a.split()[-1].lstrip("*") for a in declared] == ["solute", "params", "kij", "temp", "n", "h", "rho_vl", "p_sat", "dlnh_drho",
                                                             "status", "stream"]
    assert callable(native.mix_henry) and callable(PcSaftMix.henrys_law_constant)


def test_kernel_resources(hip_lib):
    from feos_torch_amd import build

    with open(build.RESOURCES) as f:
        res = json.load(f)
    assert "k_mix_henry" in res
    print("k_mix_henry:", res["k_mix_henry"])
    assert res["k_mix_henry"]["scratch"] <= 2304, res["k_mix_henry"]
    # the backward pass is made of existing kernels
    assert "k_mix_derivatives_vjp" in res and any("k_pure_jacobian" in name for name in res)


def test_argument_validation_without_gpu(hip_lib):
    L = hip_lib
    nul, one = None, ctypes.c_void_p(16)  # never dereferenced: the checks come first
    call = lambda solute, n, req, out: L.pcs_mix_henry(solute, req, req, req, n, out, nul, nul, nul, out, nul)
    assert call(0, 0, nul, nul) == 0 and call(1, 0, one, one) == 0  # empty batch: returns at once
    assert call(0, 5, one, nul) != 0  # h and status are required
    assert b"pcs_mix_henry" in L.pcs_last_error()
    for solute in (2, -1):
        assert call(solute, 5, one, one) != 0
        assert b"solute" in L.pcs_last_error()
    assert call(1, 5, ctypes.c_void_p(8), one) != 0
    assert b"16-byte aligned" in L.pcs_last_error()
    for n, req in ((-1, one), (1 << 31, one), (5, nul)):
        assert call(0, n, req, one) != 0, n
        assert L.pcs_last_error() != b""
    assert call(0, 0, nul, nul) == 0 and L.pcs_last_error() == b""  # a clean call clears the message


def test_public_method_checks_its_arguments_before_the_device():
    import pytest
    import torch

    from feos_torch_amd import PcSaftMix

    f64 = torch.float64
    row = [1.5, 3.5, 250.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    T = torch.tensor([300.0], dtype=f64)
    eos = PcSaftMix(torch.tensor([[row, row]], dtype=f64), torch.zeros((1, 2), dtype=f64))
    for solute in (2, -1, 0.5, True, None):
        with pytest.raises(ValueError, match="solute"):
            eos.henrys_law_constant(T, solute=solute)
    with pytest.raises(Exception, match="binary"):
        PcSaftMix(torch.tensor([[row, row, row]], dtype=f64)).henrys_law_constant(T)
