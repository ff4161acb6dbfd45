"""CPU: pcs_gc_point_jacobian and pcs_gc_point_segment_gradient (ABI 113) are exported and bound, validate their arguments
before they touch the device, and their kernels stay within the default per-lane stack limit of tests/test_abi.py."""
import ctypes
import json

import pytest

JAC, SEG = "pcs_gc_point_jacobian", "pcs_gc_point_segment_gradient"


def test_abi_version_symbols_and_bindings(hip_lib):
    from feos_torch_amd import _lib, native

    assert hip_lib.pcs_abi_version() >= 113
    for entry in (JAC, SEG):
        assert hasattr(hip_lib, entry)
        res, args = _lib.SIGNATURES[entry]
        assert res is ctypes.c_int and len(args) == 13, entry
        assert args[0] is ctypes.c_int and args[2] is ctypes.c_int and args[7] is ctypes.c_int64, entry
        assert all(a is ctypes.c_void_p for k, a in enumerate(args) if k not in (0, 2, 7)), entry
    assert callable(native.gc_point_jacobian) and callable(native.gc_point_segment_gradient)


def test_kernel_resources(hip_lib):
    from feos_torch_amd import build

    with open(build.RESOURCES) as f:
        res = json.load(f)
    new = [k for k in res if "k_gc_point_jacobian<" in k or "k_gc_segment_gradient<2," in k]
    for inst in ("k_gc_point_jacobian<true, true>", "k_gc_point_jacobian<true, false>", "k_gc_point_jacobian<false, true>",
                 "k_gc_segment_gradient<2, 192>"):
        assert any(inst in k for k in new), (inst, sorted(res))
    for k in new:
        # held to the default limit: none of the relaxed name patterns of tests/test_abi.py applies
        assert "vjp" not in k and "k_gc_segment_gradient<1," not in k and "k_mixn" not in k, k
        assert res[k]["scratch"] <= 2304, (k, res[k])
    # what serves the default backward passes: pcs_gc_jacobian launches the pressure-only instantiation (no kernel of its own)
    assert "k_gc_jacobian" not in res and any("k_gc_point_jacobian<true, false>" in k for k in res)
    assert any("k_gc_segment_gradient<0," in k for k in res)
    assert "gc_incipient.hip" in build.GUARDED_SOURCES and "gc_incipient.hip" not in build.RELAXED_SOURCES
    assert "gc_gradient.hip" not in build.GUARDED_SOURCES and "gc_gradient.hip" not in build.RELAXED_SOURCES


def test_argument_validation_without_gpu(hip_lib):
    L = hip_lib
    nul, one = None, ctypes.c_void_p(16)  # never dereferenced: the checks come first
    jac = lambda n, req, jp, jy, S=4: L.pcs_gc_point_jacobian(0, req, S, req, req, req, req, n, jp, jy, nul, nul, nul)
    seg = lambda n, req, gp, gy, S=4, out=one: L.pcs_gc_point_segment_gradient(1, req, S, req, req, req, req, n, gp, gy, out, nul, nul)
    for entry, call, a, b in ((JAC, jac, b"jac_p", b"jac_y"), (SEG, seg, b"gout_p", b"gout_y")):
        assert call(0, nul, nul, nul) == 0 and call(0, one, one, one) == 0  # empty batch: returns at once
        assert call(5, one, nul, nul) != 0  # both outputs / both weights NULL
        msg = L.pcs_last_error()
        assert entry.encode() in msg and a in msg and b in msg, msg
        for n, req in ((-1, one), (1 << 31, one), (5, nul)):
            assert call(n, req, one, one) != 0, (entry, n)
            assert entry.encode() in L.pcs_last_error(), (entry, n, L.pcs_last_error())
        assert call(-1, one, one, one) != 0 and b"n must" in L.pcs_last_error()
        for S in (0, 33):
            assert call(5, one, one, one, S=S) != 0
            assert entry.encode() in L.pcs_last_error() and b"S, the number of segment types" in L.pcs_last_error()
        assert call(0, nul, nul, nul) == 0 and L.pcs_last_error() == b""  # a clean call clears the message
    assert seg(5, one, one, one, out=nul) != 0 and b"grad_seg" in L.pcs_last_error()
    # rows must be 16-byte aligned like every gc entry point
    odd = ctypes.c_void_p(24)
    assert L.pcs_gc_point_jacobian(0, one, 4, odd, one, one, one, 5, one, one, nul, nul, nul) != 0
    assert b"aligned" in L.pcs_last_error()
    assert jac(0, nul, nul, nul) == 0 and L.pcs_last_error() == b""  # leave no message behind for the tests that follow


def test_wrappers_validate_on_the_host():
    import torch

    from feos_torch_amd import native

    f64 = torch.float64
    S = 3
    table = torch.zeros(S * 8 + 3 * S * S, dtype=f64)
    rows = torch.zeros((4, 80), dtype=torch.uint8)
    phi, T, rho4 = torch.ones((4, 2), dtype=f64), torch.ones(4, dtype=f64), torch.ones((4, 4), dtype=f64)
    with pytest.raises(ValueError, match="want_p / want_y"):
        native.gc_point_jacobian(table, S, rows, phi, T, rho4, False, want_p=False, want_y=False)
    with pytest.raises(ValueError, match="gout_p / gout_y"):
        native.gc_point_segment_gradient(table, S, rows, phi, T, rho4, False)
    with pytest.raises(ValueError, match="rho4 has 3 rows, expected 4"):
        native.gc_point_jacobian(table, S, rows, phi, T, rho4[:3], False)
    with pytest.raises(ValueError, match="gout_y has 2 rows, expected 4"):
        native.gc_point_segment_gradient(table, S, rows, phi, T, rho4, False, gout_y=T[:2])
    with pytest.raises(ValueError, match="table must be"):
        native.gc_point_segment_gradient(table[:-1], S, rows, phi, T, rho4, False, gout_p=T)
