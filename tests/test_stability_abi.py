"""CPU: the C ABI of the stability analysis (pcs_mix_stability / pcs_gc_stability) -- argument checks before any device
work, the ABI version, the compiler's resource report of the two kernels -- and the binary-only guard of
PcSaftMix.stability_analysis."""
import ctypes
import inspect
import json

import pytest


def test_argument_validation_without_gpu(hip_lib):
    L = hip_lib
    nul = None
    one = ctypes.c_void_p(16)  # never dereferenced: the checks come first
    calls = {
        "pcs_mix_stability": lambda n, st: L.pcs_mix_stability(one, one, one, one, n, nul, nul, st, nul),
        "pcs_gc_stability": lambda n, st: L.pcs_gc_stability(one, 4, one, one, one, one, n, nul, nul, st, nul, nul),
    }
    for name, call in calls.items():
        assert call(0, one) == 0, name  # empty batch: a no-op
        for n, st in ((-1, one), (1 << 31, one), (5, nul)):
            assert call(n, st) != 0, (name, n)
            assert L.pcs_last_error() != b"", (name, n)
    assert L.pcs_mix_stability(one, one, one, nul, 5, one, one, one, nul) != 0 and b"null" in L.pcs_last_error()
    assert L.pcs_gc_stability(one, 0, one, one, one, one, 5, nul, nul, one, nul, nul) != 0  # S out of range


def test_abi_version(hip_lib):
    assert hip_lib.pcs_abi_version() >= 105


def test_kernel_resources(hip_lib):
    from feos_torch_amd import build

    with open(build.RESOURCES) as f:
        res = json.load(f)
    for name in ("k_mix_stability", "k_gc_stability"):
        assert name in res, sorted(res)
        assert res[name]["scratch"] <= 2304, (name, res[name])
        # held to the default stack limit of tests/test_abi.py (none of its relaxed name patterns applies)
        assert not any(pat in name for pat in ("vjp", "k_mixn", "k_gc_segment_gradient<1,")), name
    assert "stability_kernels.hip" in build.GUARDED_SOURCES  # IEEE NaN / inf semantics for the outcome logic


def test_binary_only_before_any_device_call(monkeypatch):
    import torch

    from feos_torch_amd import PcSaftMix, native

    def boom(*a, **k):
        raise AssertionError("device call")

    monkeypatch.setattr(native, "mix_stability", boom)
    monkeypatch.setattr(native, "_dev", boom)
    par = torch.tensor([[1.5, 3.5, 250.0, 0, 0, 0, 0, 0]] * 3, dtype=torch.float64).repeat(2, 1, 1)  # [2,3,8]
    eos = PcSaftMix(par)
    with pytest.raises(Exception, match="binary"):
        eos.stability_analysis(torch.tensor([300.0, 300.0], dtype=torch.float64), torch.full((2, 3), 1e-3, dtype=torch.float64))


def test_wrappers_validate_rows_host_side():
    from feos_torch_amd import native

    for name in ("mix_stability", "gc_stability"):
        src = inspect.getsource(getattr(native, name))
        assert "_same_rows(" in src, name
