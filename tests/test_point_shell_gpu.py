"""The shell of the bubble / dew point properties added after tests/golden/model_shell.json was recorded, pinned bit for
bit like tests/test_model_shell_gpu.py pins the others: PcSaftMix.bubble_point / dew_point with incipient_molefracs=True,
PcSaftMix.bubble_temperature / dew_temperature (with and without the incipient composition) and
GcPcSaftMix.bubble_temperature / dew_temperature, each with and without check_stability, with all five rows solving (batch
"a") and with row 2 dropped (batch "b").

The recorded bits (tests/golden/point_shell.json, written by tests/golden/make_golden_point_shell.py, which drives the
runner of this module) are those of commit f1a565d, the last one with one autograd Function per property.  Inputs: the mix
and gc rows of model_shell.json; a temperature call is given the pressure that model_shell.json records for the matching
bubble / dew case and starts 2 % below the recorded temperature; batch "b" of a temperature call has p_spec[2] = -1.

Per case and batch: the values (T or p, and y), nans, stable, a second call on the reduced model; per backward pass (through
the value; for the incipient cases also through y alone and through both with different weights) every gradient; and the
ordered list of C-ABI entry points the forward pass and, per gradient pattern ("parameters", the third differentiable input,
"all") and backward pass, the backward pass went through (a wrapper around native._call for the duration of the run): same
kernels, same order, none added.  On f1a565d a gradient has the same bits under every pattern that asks for it and the
forward pass makes the same calls under all three (the generator asserts both), so the file holds each once -- one string
of 16 hex digits per entry for every tensor -- and every pattern is compared with it.  Comparison rule of tests/test_model_shell_gpu.py: everything bit for bit, on "cpu" and on "cuda",
except the two gradients that are sums over the rows (gc segment parameters, gc k_ab): ten times the spread of two runs of
f1a565d, at least 4 ulp of the largest entry, and bit for bit where those two runs agreed."""
import contextlib
import os
import sys

import pytest
import torch

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_model_shell_gpu import (BAD_ROW, N, SUMMED, _check_gradient, _gc_grads, _gc_model, _Leaves, _weights,  # noqa: E402
                                  from_hex, prop_key, same_bits, to_hex, with_bad_row)

pytestmark = pytest.mark.gpu
f64 = torch.float64

START = 0.98  # first iterate of a temperature call / the recorded temperature
# (family, solved quantity, dew, check_stability, incipient_molefracs)
CASES = [("mix", "pressure", dew, check, True) for dew in (False, True) for check in (False, True)] + \
        [("mix", "temperature", dew, check, inc) for dew in (False, True) for check in (False, True) for inc in (False, True)] + \
        [("gc", "temperature", dew, check, False) for dew in (False, True) for check in (False, True)]
BACKWARDS = ("value", "y", "both")  # which outputs the backward pass starts from ("y", "both": incipient cases)


def pack(t):
    return "".join(to_hex(t))


def split16(s):
    return [s[i:i + 16] for i in range(0, len(s), 16)]


def unpack(s, shape=None):
    return from_hex(split16(s), shape)


def case_key(case):
    family, solved, dew, check, inc = case
    return f"{family}/{'dew' if dew else 'bubble'}_{solved}{'+stability' if check else ''}{'+incipient' if inc else ''}"


def patterns(case):
    """parameters only, the third differentiable input only (temperature of a pressure call, pressure of a temperature
    call), all"""
    return ("parameters", "temperature" if case[1] == "pressure" else "pressure", "all")


def backwards(case):
    return BACKWARDS if case[4] else BACKWARDS[:1]


def make_inputs(model_shell):
    """What goes into point_shell.json["inputs"]: the mix and gc rows of model_shell.json and, per temperature case, the
    pressure it records for the matching bubble / dew case of batch "a"."""
    p_spec = {case_key(c): from_hex(model_shell["properties"][f"{prop_key(c[0], (c[2], c[3]))}/a"]["values"][0]).tolist()
              for c in CASES if c[1] == "temperature"}
    return {"mix": model_shell["inputs"]["mix"], "gc": model_shell["inputs"]["gc"], "p_spec": p_spec, "start": START}


def case_inputs(inputs, case, batch):
    """The rows of one case and batch: `temperature`, `molefracs`, `pressure` hold the call's three arguments by meaning (for
    a temperature call: the first iterate and p_spec)."""
    inp = dict(inputs[case[0]])
    if case[1] == "pressure":
        return inp if batch == "a" else with_bad_row(inp, case[0])
    inp["temperature"] = [inputs["start"] * T for T in inp["temperature"]]
    inp["pressure"] = list(inputs["p_spec"][case_key(case)])
    if batch == "b":
        inp["pressure"][BAD_ROW] = -1.0
    return inp


@contextlib.contextmanager
def recorded_calls():
    """Names of the C-ABI entry points that go through native._call while the block runs, in order."""
    from feos_torch_amd import native

    names, real = [], native._call

    def spy(device, name, *args):
        names.append(name)
        return real(device, name, *args)

    native._call = spy
    try:
        yield names
    finally:
        native._call = real


class _Blind(torch.autograd.Function):
    """Uses its input and hands no gradient back: the node before it runs its backward with every upstream gradient absent."""

    @staticmethod
    def forward(ctx, x):
        return x.sum()

    @staticmethod
    def backward(ctx, g):
        return None


def _y_weights(v):
    return 2.0 - 0.125 * torch.arange(v.shape[0], dtype=f64, device=v.device)


def run_point(amd, case, inp, device, pattern, backward):
    """One point-property call on fresh leaves and one backward pass (backward: "value", "y", "both", or "neither" for a
    pass that reaches the Function with no upstream gradient) -> dict(values, nans, stable, grads, required, second, calls)."""
    family, solved, dew, check, inc = case
    leaf = _Leaves(device, pattern, {"mix": ("parameters", "kij"), "gc": tuple(f"segment{k}" for k in range(8))}[family])
    if family == "mix":
        model = amd.PcSaftMix(leaf("parameters", inp["parameters"]), leaf("kij", inp["kij"]))
        rows = lambda: (model._par.shape[0], model.kij.shape[0])
    else:
        model = _gc_model(amd, inp, leaf)
        rows = lambda: (model.rows.shape[0], model.phi.shape[0])
    T, x, p = (leaf(name, inp[name]) for name in ("temperature", "molefracs", "pressure"))
    method = getattr(model, ("dew_" if dew else "bubble_") + ("point" if solved == "pressure" else "temperature"))
    args = (T, x, p) if solved == "pressure" else (p, x, T)
    kwargs = dict(check_stability=True) if check else {}
    if inc:
        kwargs["incipient_molefracs"] = True
    with recorded_calls() as calls:
        out = method(*args, **kwargs)
        assert len(out) == 2 + check + inc
        values, nans = [out[0]] + ([out[-1]] if inc else []), out[1]
        stable = out[2] if check else None
        n_ok = int((~nans).sum())
        required = {name[:7] if name.startswith("segment") else name for name, t in leaf.leaves.items() if t.requires_grad}
        assert all(v.requires_grad for v in values) and required  # every pattern reaches something the value depends on
        forward_calls = len(calls)
        if backward == "neither":
            _Blind.apply(values[0]).backward()
        else:
            loss = (_weights(values[0]) * values[0]).sum() if backward != "y" else 0.0
            if backward != "value":
                loss = loss + (_y_weights(values[1]) * values[1]).sum()
            loss.backward()
    for t in values + [nans] + ([stable] if check else []):
        assert t.device.type == device
    assert nans.dtype == torch.bool and nans.shape == (N,) and all(v.shape == (n_ok,) and v.dtype == f64 for v in values)
    assert stable is None or (stable.dtype == torch.bool and stable.shape == (n_ok,) and not stable.requires_grad)
    assert not nans.requires_grad and rows() == (n_ok, n_ok)  # the call reduced the model
    grads = _gc_grads(leaf) if family == "gc" else leaf.grads()
    # a second call on the reduced model with the reduced inputs
    keep = ~nans
    second = method(*[a.detach()[keep] for a in args], **kwargs)
    assert second[1].shape == (n_ok,) and not bool(second[1].any())
    second = [second[0]] + ([second[-1]] if inc else [])
    assert all(v.shape == (n_ok,) and v.device.type == device for v in second)
    return {"values": values, "nans": nans, "stable": stable, "grads": grads, "required": required, "second": second,
            "forward_calls": calls[:forward_calls], "backward_calls": calls[forward_calls:]}


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def amd():
    assert torch.cuda.is_available()
    import feos_torch_amd

    return feos_torch_amd


@pytest.fixture(scope="module")
def gold():
    return load_golden("point_shell.json")


def test_inputs_are_those_of_the_model_shell(gold):
    assert gold["commit"] == "f1a565d" and gold["inputs"] == make_inputs(load_golden("model_shell.json"))
    assert sorted(gold["cases"]) == sorted(f"{case_key(c)}/{b}" for c in CASES for b in "ab") and len(CASES) == 16


@pytest.mark.parametrize("case", CASES, ids=[case_key(c) for c in CASES])
def test_point_shell(amd, gold, case):
    for batch in ("a", "b"):
        inp = case_inputs(gold["inputs"], case, batch)
        rec = gold["cases"][f"{case_key(case)}/{batch}"]
        want_nans = [batch == "b" and i == BAD_ROW for i in range(N)]
        assert rec["nans"] == want_nans
        for device in ("cpu", "cuda"):
            for pattern in patterns(case):
                for backward in backwards(case):
                    r = run_point(amd, case, inp, device, pattern, backward)
                    want_grads = rec["grads"][backward]  # of the inputs the outputs depend on
                    assert r["nans"].tolist() == want_nans
                    for got, want in ((r["values"], rec["values"]), (r["second"], rec["second"])):
                        assert len(got) == len(want)
                        for v, h in zip(got, want):  # the same bits whatever requires a gradient, wherever the inputs live
                            assert same_bits(v, unpack(h))
                    assert (r["stable"].tolist() if case[3] else None) == rec["stable"]
                    assert r["forward_calls"] == rec["forward_calls"], (pattern, backward)
                    assert r["backward_calls"] == rec["backward_calls"][f"{pattern}/{backward}"], (pattern, backward)
                    for name, g in r["grads"].items():
                        expected = name in want_grads and name in r["required"]
                        assert (g is not None) == expected, (name, pattern, backward)
                        if g is not None:
                            want = want_grads[name]
                            _check_gradient(name, g, {"hex": split16(want["hex"]), "spread": want["spread"]})
                            if batch == "b" and name not in SUMMED:
                                assert not bool(g[BAD_ROW].any())  # exactly zero in the dropped row
            if case[4]:  # a backward pass that reaches neither the value nor y: no gradient anywhere, no kernel
                r = run_point(amd, case, inp, device, "all", "neither")
                assert all(g is None for g in r["grads"].values()) and r["backward_calls"] == []
