"""CPU: pcs_mix_point_jacobian (ABI 111) is exported and bound, validates its arguments before it touches the device, and
its kernel stays within the per-lane stack limit of tests/test_abi.py."""
import ctypes
import json


def test_abi_version_symbol_and_binding(hip_lib):
    from feos_torch_amd import _lib, native

    assert hip_lib.pcs_abi_version() >= 111
    assert hasattr(hip_lib, "pcs_mix_point_jacobian")
    res, args = _lib.SIGNATURES["pcs_mix_point_jacobian"]
    assert res is ctypes.c_int and len(args) == 10 and args[0] is ctypes.c_int and args[5] is ctypes.c_int64
    assert callable(native.mix_point_jacobian)


def test_kernel_resources(hip_lib):
    from feos_torch_amd import build

    with open(build.RESOURCES) as f:
        res = json.load(f)
    assert "k_mix_point_jacobian" in res
    assert res["k_mix_point_jacobian"]["scratch"] <= 2304, res["k_mix_point_jacobian"]
    assert "k_mix_jacobian" in res  # the default backward pass is still there


def test_argument_validation_without_gpu(hip_lib):
    L = hip_lib
    nul, one = None, ctypes.c_void_p(16)  # never dereferenced: the checks come first
    call = lambda n, req, jp, jy: L.pcs_mix_point_jacobian(0, req, req, req, req, n, jp, jy, nul, nul)
    assert call(0, nul, nul, nul) == 0 and call(0, one, one, one) == 0  # empty batch: returns at once
    assert call(5, one, nul, nul) != 0  # both outputs NULL
    msg = L.pcs_last_error()
    assert b"pcs_mix_point_jacobian" in msg and b"jac_p" in msg and b"jac_y" in msg, msg
    for n, req in ((-1, one), (1 << 31, one), (5, nul)):
        assert call(n, req, one, one) != 0, n
        assert L.pcs_last_error() != b""
    assert call(0, nul, nul, nul) == 0 and L.pcs_last_error() == b""  # a clean call clears the message
