"""CPU: pcs_gc_density (ABI 115) is declared, exported and bound with one signature, validates its arguments before it touches
the device, and its kernel keeps its one evaluation site in registers (scratch <= 256 B per lane)."""
import ctypes
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbol_and_binding_agree(hip_lib):
    from feos_torch_amd import GcPcSaftMix, _lib, native

    assert hip_lib.pcs_abi_version() >= 115
    assert hasattr(hip_lib, "pcs_gc_density")
    with open(os.path.join(ROOT, "include", "pcsaft_hip.h")) as f:
        header = f.read()
    m = re.search(r"int pcs_gc_density\(([^)]*)\);", header)
    assert m, "pcs_gc_density is not declared in include/pcsaft_hip.h"
    declared = [" ".join(a.split()) for a in m.group(1).split(",")]
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    want = [ctypes.c_void_p if "*" in a else kinds[a.split()[0]] for a in declared]
    res, args = _lib.SIGNATURES["pcs_gc_density"]
    assert res is ctypes.c_int and list(args) == want, (declared, args)
    assert [a.split()[-1].lstrip("*") for a in declared] == ["phase", "table", "S", "rows", "phi", "temp", "pressure", "x", "n", "rho",
                                                             "dpdrho", "status", "iters", "order", "stream"]
    assert callable(native.gc_density)
    assert callable(GcPcSaftMix.liquid_density) and callable(GcPcSaftMix.vapor_density)


def test_kernel_resources(hip_lib):
    from feos_torch_amd import build

    with open(build.RESOURCES) as f:
        res = json.load(f)
    assert "k_gc_density" in res
    print("k_gc_density:", res["k_gc_density"])
    assert res["k_gc_density"]["scratch"] <= 256, res["k_gc_density"]
    assert any("k_gc_segment_gradient<1" in k for k in res), "the backward pass is the existing VJP kernel"


def test_argument_validation_without_gpu(hip_lib):
    L = hip_lib
    nul, one = None, ctypes.c_void_p(16)  # never dereferenced: the checks come first
    call = lambda phase, S, n, req, status: L.pcs_gc_density(phase, req, S, req, req, req, req, req, n, nul, nul, status, nul, nul, nul)
    assert call(0, 23, 0, nul, nul) == 0 and call(1, 23, 0, one, one) == 0  # empty batch: returns at once
    assert call(0, 23, 5, one, nul) != 0  # status is required
    assert b"pcs_gc_density" in L.pcs_last_error()
    for phase in (2, -1):
        assert call(phase, 23, 5, one, one) != 0
        assert b"phase" in L.pcs_last_error()
    for S in (0, 33, -1):
        assert call(0, S, 5, one, one) != 0, S
        assert b"[1, 32]" in L.pcs_last_error()
    assert call(0, 23, 5, ctypes.c_void_p(8), one) != 0
    assert b"16-byte aligned" in L.pcs_last_error()
    for n, req in ((-1, one), (1 << 31, one), (5, nul)):
        assert call(0, 23, n, req, one) != 0, n
        assert L.pcs_last_error() != b""
    assert call(0, 23, 0, nul, nul) == 0 and L.pcs_last_error() == b""  # a clean call clears the message
