"""The shell of the model classes in one place: devices, shapes, tuple orders, model reduction, which inputs receive a
gradient, and the bits of every value and gradient -- for every property of PcSaftPure, PcSaftMix and GcPcSaftMix with all
rows converging (batch "a") and with row 2 dropped (batch "b"), for the four state-function paths, and for
native.Compaction / native.PureVlePlan.

The recorded bits (tests/golden/model_shell.json, written by tests/golden/make_golden_model_shell.py, which drives the
runners of this module) are those of commit a55be04: the Python layer above the kernels was rewritten after it and
must not change a bit.  Everything is compared bit for bit except the two gradients that are sums over the rows (gc
segment parameters: fp64 atomics; gc k_ab: a matrix product): ten times the spread of two runs of a55be04, at least 4 ulp of
the largest entry -- and bit for bit where those two runs agreed (the recorded spread is 0 for every case: the 3 to 5 rows
of a case are reduced by a single wavefront in a fixed order)."""
import os
import struct
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu
f64 = torch.float64

PURE = ("vapor_pressure", "liquid_density", "equilibrium_liquid_density", "critical_point")
MIX = [(dew, check) for dew in (False, True) for check in (False, True)]
PATTERNS = ("parameters", "temperature", "all")
SUMMED = ("segment", "kab")  # gradients reduced over the rows
N, BAD_ROW = 5, 2


def to_hex(t):
    return [struct.pack(">d", v).hex() for v in t.detach().cpu().double().reshape(-1).tolist()]


def from_hex(h, shape=None):
    t = torch.tensor([struct.unpack(">d", bytes.fromhex(s))[0] for s in h], dtype=f64)
    return t if shape is None else t.reshape(shape)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def segment_table():
    from feos_torch_amd.synthetic import load_segment_table

    table = load_segment_table(os.path.join(ROOT, "tests", "data", "sauer2014_hetero.json"))
    return table, [s for s, _ in table], [[float(v[k]) for _, v in table] for k in range(8)]


def make_inputs():
    """Rows of the benchmark distributions (feos_torch_amd.synthetic); batch b = batch a with row 2 made hopeless the way
    tests/test_mix_gpu.py::test_bad_rows_fail_cleanly does (T = -10 K; above T_c for the two saturation properties -- a
    super-critical isotherm still has a density root at every pressure, so liquid_density takes T = -10 K as well; a NaN
    parameter for critical_point)."""
    from feos_torch_amd.synthetic import gc_batch, mix_batch, pure_batch, pure_pressures

    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import critical_referee as cr

    P, T = pure_batch(N, seed=7)
    Pm, K, Tm, X, PI = mix_batch(N, seed=7)
    g = gc_batch(N, segment_table()[0], seed=7)
    P9 = pure_batch(9, seed=11)[0].reshape(3, 3, 8).copy()
    P9[:, 1:, 4:] = 0.0  # one associating component at most
    lst = lambda a: np.asarray(a, dtype=np.float64).tolist()
    return {
        "pure": {"parameters": lst(P), "temperature": lst(T), "pressure": lst(pure_pressures(N, seed=8)),
                 "initial_temperature": lst(cr.fit_temperature(P)), "density": [1e-3, 5e-3, 8e-3]},
        "mix": {"parameters": lst(Pm), "kij": lst(K), "temperature": lst(Tm), "molefracs": lst(X), "pressure": lst(PI),
                "density": [[2e-3, 3e-3], [1e-4, 5e-3], [4e-3, 1e-5]]},
        "mixn": {"parameters": lst(P9), "temperature": [300.0, 350.0, 400.0],
                 "density": [[1e-3, 2e-3, 5e-4], [2e-5, 1e-5, 3e-5], [3e-3, 1e-4, 1e-3]]},
        "gc": {"segment_lists": g["segment_lists"], "bond_lists": g["bond_lists"], "kab_pairs": [list(k[:2]) for k in g["kab_list"]],
               "kab": lst([k[2] for k in g["kab_list"]]), "phi": lst(g["phi"]), "temperature": lst(g["T"]), "molefracs": lst(g["x"]),
               "pressure": lst(g["p_init"]), "density": [[2e-3, 1e-3], [1e-5, 2e-5], [5e-4, 3e-3]]},
    }


def with_bad_row(inp, family, prop=None):
    inp = {k: (list(v) if isinstance(v, list) else v) for k, v in inp.items()}
    if prop == "critical_point":
        inp["parameters"] = [list(r) for r in inp["parameters"]]
        inp["parameters"][BAD_ROW][0] = float("nan")
    elif family == "pure" and prop != "liquid_density":
        inp["temperature"][BAD_ROW] *= 3.0
    else:
        inp["temperature"][BAD_ROW] = -10.0
    return inp


class _Leaves:
    """Leaf tensors of one call on one device; `pattern` decides which of them require a gradient."""

    def __init__(self, device, pattern, parameter_names):
        self.device, self.pattern, self.parameter_names, self.leaves = device, pattern, parameter_names, {}

    def __call__(self, name, data):
        grad = self.pattern == "all" or (name in self.parameter_names if self.pattern == "parameters" else name == self.pattern)
        self.leaves[name] = t = torch.tensor(data, dtype=f64, device=self.device, requires_grad=grad)
        return t

    def grads(self):
        out = {}
        for name, t in self.leaves.items():
            out[name] = t.grad
            assert t.grad is None or (t.grad.device.type == self.device and t.grad.shape == t.shape), name
        return out


def _weights(v):
    return 1.0 + 0.25 * torch.arange(v.shape[0], dtype=f64, device=v.device)


def _gc_model(amd, inp, leaf, n=None):
    _, ident, seg = segment_table()
    segs = [leaf(f"segment{k}", seg[k]) for k in range(8)]
    kab = leaf("kab", inp["kab"])
    phi = leaf("phi", inp["phi"][:n])
    return amd.GcPcSaftMix(ident, segs, inp["segment_lists"][:n], inp["bond_lists"][:n],
                           [(s1, s2, kab[i]) for i, (s1, s2) in enumerate(inp["kab_pairs"])], phi)


def _gc_grads(leaf):
    g = leaf.grads()
    seg = [g.pop(f"segment{k}") for k in range(8)]
    assert len({s is None for s in seg}) == 1
    g["segment"] = None if seg[0] is None else torch.stack(seg, dim=1)
    return g


def run_property(amd, family, prop, inp, device, pattern):
    """One property call on fresh leaves -> dict(values, nans, stable, grads {input: tensor or None}, rows, second)."""
    names = {"pure": ("parameters",), "mix": ("parameters", "kij"), "gc": tuple(f"segment{k}" for k in range(8))}
    leaf = _Leaves(device, pattern, names[family])
    stable = None
    if family == "pure":
        model = amd.PcSaftPure(leaf("parameters", inp["parameters"]))
        if prop == "critical_point":
            args = (torch.tensor(inp["initial_temperature"], dtype=f64, device=device),)  # never receives a gradient
        else:
            args = (leaf("temperature", inp["temperature"]),) + ((leaf("pressure", inp["pressure"]),) if prop == "liquid_density" else ())
        nans, *values = getattr(model, prop)(*args)
        rows = lambda: model._par.shape[0]
    else:
        dew, check = prop
        if family == "mix":
            model = amd.PcSaftMix(leaf("parameters", inp["parameters"]), leaf("kij", inp["kij"]))
            rows = lambda: (model._par.shape[0], model.kij.shape[0])
        else:
            model = _gc_model(amd, inp, leaf)
            rows = lambda: (model.rows.shape[0], model.phi.shape[0])
        args = (leaf("temperature", inp["temperature"]), leaf("molefracs", inp["molefracs"]), leaf("pressure", inp["pressure"]))
        out = (model.dew_point if dew else model.bubble_point)(*args, **({"check_stability": True} if check else {}))
        assert len(out) == (3 if check else 2)
        values, nans = [out[0]], out[1]
        stable = out[2] if check else None
    n_ok = int((~nans).sum())
    for t in values + [nans] + ([stable] if stable is not None else []):
        assert t.device.type == device
    assert nans.dtype == torch.bool and nans.shape == (N,) and all(v.shape == (n_ok,) and v.dtype == f64 for v in values)
    assert stable is None or (stable.dtype == torch.bool and stable.shape == (n_ok,))
    assert not nans.requires_grad and (stable is None or not stable.requires_grad)
    after = rows()
    assert after == n_ok or after == (n_ok, n_ok)  # the call reduced the model
    required = {name[:7] if name.startswith("segment") else name for name, t in leaf.leaves.items() if t.requires_grad}
    assert values[0].requires_grad == bool(required)
    if required:
        sum((_weights(v) * v).sum() for v in values).backward()
    grads = _gc_grads(leaf) if family == "gc" else leaf.grads()
    # a second call on the reduced model with the reduced inputs
    keep = ~nans
    second = getattr(model, prop)(*[a.detach()[keep] for a in args]) if family == "pure" else \
        (model.dew_point if dew else model.bubble_point)(*[a.detach()[keep] for a in args])
    nans2, value2 = (second[0], second[1]) if family == "pure" else (second[1], second[0])
    assert nans2.shape == (n_ok,) and value2.shape == (n_ok,) and value2.device.type == device
    return {"values": values, "nans": nans, "stable": stable, "grads": grads, "required": required, "second": value2, "second_nans": nans2}


DERIV_FAMILIES = ("pure", "mix", "mixn", "gc")


def run_derivatives(amd, family, inp, device, only=None):
    """The state functions at n = 3 on fresh leaves, every input requiring a gradient; backward of sum_k (k + 1) sum(out_k)
    (only = k: of sum(out_k) alone, so that the other outputs' upstream gradients are None) -> (outputs, grads)."""
    n = 3
    leaf = _Leaves(device, "all", ())
    cut = lambda key: inp[key][:n]
    if family == "pure":
        model = amd.PcSaftPure(leaf("parameters", cut("parameters")))
    elif family == "mix":
        model = amd.PcSaftMix(leaf("parameters", cut("parameters")), leaf("kij", cut("kij")))
    elif family == "mixn":
        model = amd.PcSaftMix(leaf("parameters", cut("parameters")))
    else:
        model = _gc_model(amd, inp, leaf, n)
    out = model.derivatives(leaf("temperature", cut("temperature")), leaf("density", cut("density")))
    assert len(out) == (3 if family == "pure" else 4)
    ncomp = {"pure": None, "mix": 2, "mixn": 3, "gc": 2}[family]
    for k, o in enumerate(out):
        assert o.device.type == device and o.dtype == f64
        assert o.shape == ((n,) if (k < 2 or family == "pure") else (n, ncomp))
    (out[only].sum() if only is not None else sum((k + 1.0) * o.sum() for k, o in enumerate(out))).backward()
    grads = _gc_grads(leaf) if family == "gc" else leaf.grads()
    assert all(g is not None for g in grads.values())  # the state functions depend on every input
    return list(out), grads


def run_compaction(native):
    """native.Compaction through every method, one dropped row of five (and the all-kept plan) -> dict of tensors."""
    dev = "cuda"
    ar = lambda *shape: (torch.arange(int(np.prod(shape)), dtype=f64, device=dev).reshape(shape) + 1.0) / 7.0
    drop = torch.tensor([False, False, True, False, False], device=dev)
    comp = native.Compaction(drop)
    assert (comp.n, comp.n_ok, comp.all_ok) == (5, 4, False) and comp.status.dtype == torch.uint8 and comp.cws.dtype == torch.int32
    u8 = (torch.arange(5 * 16, device=dev) % 251).to(torch.uint8).reshape(5, 16)
    src, g, v = ar(4, 10), ar(4) + 2.0, ar(4) * 3.0
    out = {"gather1": comp.gather(ar(5)), "gather2": comp.gather(ar(5, 3)), "gather_u8": comp.gather(u8).to(f64),
           "index": comp.index().to(f64), "expand_g": comp.expand(src, g, 1, 8), "expand_col": comp.expand(src, None, 9, 1),
           "expand_1d": comp.expand(v)}
    assert out["gather2"].shape == (4, 3) and out["gather_u8"].shape == (4, 16) and out["expand_g"].shape == (5, 8)
    assert out["expand_col"].shape == (5, 1) and out["expand_1d"].shape == (5,)
    full = native.Compaction(torch.zeros(5, dtype=torch.uint8, device=dev))
    assert full.all_ok and full.n_ok == 5
    x = ar(5, 2)
    assert full.gather(x) is x
    out["full_index"] = full.index().to(f64)
    out["full_expand"] = full.expand(ar(5, 10), ar(5), 8, 2)
    out["rows"] = native.compact_rows(comp, ar(5, 8))
    with pytest.raises(ValueError, match="tensor has 4 rows, the mask 5"):
        comp.gather(ar(4))
    with pytest.raises(ValueError, match="one row per kept row"):
        comp.expand(ar(5, 10))
    return out


def run_plan(native, inp):
    """native.PureVlePlan through every method on batch b of the pure rows -> dict of tensors."""
    par = torch.tensor(inp["parameters"], dtype=f64, device="cuda")
    T = torch.tensor(inp["temperature"], dtype=f64, device="cuda")
    out = {}
    for fp64 in (False, True):
        plan = native.PureVlePlan(N, "cuda", want_rho_eq=True, want_rho_vl=True, all_fp64=fp64)
        for method in ("run",) if fp64 else ("run", "run_fast", "run_retry"):
            if method != "run_retry":  # run_retry finishes what run_fast left
                for t in (plan.p_sat, plan.rho_eq, plan.rho_vl, plan.status):
                    t.zero_()
            getattr(plan, method)(par, T)
            key = f"{method}{'_fp64' if fp64 else ''}"
            for name in ("p_sat", "rho_eq", "rho_vl", "status"):
                out[f"{key}/{name}"] = getattr(plan, name).to(f64)
            out[f"{key}/retry_count"] = torch.tensor(plan.retry_count(), dtype=f64)
    return out


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def amd():
    assert torch.cuda.is_available()
    import feos_torch_amd

    return feos_torch_amd


@pytest.fixture(scope="module")
def gold():
    return load_golden("model_shell.json")


def _np(inp, *keys):
    return [np.array(inp[k], dtype=np.float64) for k in keys]


def _oracle_status(oracle, family, prop, inp):
    if family == "pure":
        P, T, p = _np(inp, "parameters", "temperature", "pressure")
        if prop == "critical_point":
            sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
            import critical_referee as cr

            bad = np.isnan(P).any(axis=1)
            st = bad.copy()
            st[~bad] = ~np.isfinite(cr.oracle_scan(oracle, P[~bad])[0])
            return st
        if prop == "liquid_density":
            return oracle.pure_liquid_density(P, T, p)[1]
        return (oracle.pure_vapor_pressure if prop == "vapor_pressure" else oracle.pure_equilibrium_liquid_density)(P, T)[1]
    if family == "mix":
        return oracle.mix_bubble_dew(*_np(inp, "parameters", "kij", "temperature", "molefracs", "pressure"), prop[0])[2]
    kab = [(s1, s2, k) for (s1, s2), k in zip(inp["kab_pairs"], inp["kab"])]
    enc = oracle.gc_encode(segment_table()[0], inp["segment_lists"], inp["bond_lists"], kab)
    return oracle.gc_bubble_dew(enc, *_np(inp, "phi", "temperature", "molefracs", "pressure"), prop[0])[2]


def _check_gradient(name, got, rec):
    want = from_hex(rec["hex"], got.shape)
    if name in SUMMED and rec["spread"] > 0.0:
        tol = max(10.0 * rec["spread"], 4.0 * float(np.spacing(float(want.abs().max()))))
        assert float((got.cpu() - want).abs().max()) <= tol, name
    else:
        assert same_bits(got, want), name


def prop_key(family, prop):
    return f"{family}/{prop}" if family == "pure" else f"{family}/{'dew' if prop[0] else 'bubble'}{'+stability' if prop[1] else ''}"


CASES = [("pure", p) for p in PURE] + [(f, p) for f in ("mix", "gc") for p in MIX]


@pytest.mark.parametrize("family,prop", CASES, ids=[prop_key(*c) for c in CASES])
def test_property_shell(amd, oracle, gold, family, prop):
    for batch in ("a", "b"):
        inp = gold["inputs"][family] if batch == "a" else with_bad_row(gold["inputs"][family], family, prop)
        want_nans = [batch == "b" and i == BAD_ROW for i in range(N)]
        assert _oracle_status(oracle, family, prop, inp).tolist() == want_nans  # both branches of the shell are really taken
        rec = gold["properties"][f"{prop_key(family, prop)}/{batch}"]
        for device in ("cpu", "cuda"):
            for pattern in PATTERNS:
                r = run_property(amd, family, prop, inp, device, pattern)
                assert r["nans"].tolist() == want_nans and not bool(r["second_nans"].any())
                for v, h in zip(r["values"], rec["values"]):  # the same bits whatever requires a gradient, wherever the inputs live
                    assert same_bits(v, from_hex(h))
                assert same_bits(r["second"], from_hex(rec["second"]))
                if prop in MIX and prop[1]:
                    assert r["stable"].tolist() == rec["stable"]
                depends = [k for k in rec["grads"]]  # inputs the value depends on; the others never receive a gradient
                for name, g in r["grads"].items():
                    expected = name in depends and name in r["required"]
                    assert (g is not None) == expected, (name, pattern)
                    if g is not None:
                        _check_gradient(name, g, rec["grads"][name])
                        if batch == "b" and name not in SUMMED:
                            assert not bool(g[BAD_ROW].any())  # exactly zero in the dropped row


@pytest.mark.parametrize("family", DERIV_FAMILIES)
def test_state_function_shell(amd, gold, family):
    rec = gold["derivatives"][family]
    for device in ("cpu", "cuda"):
        for only in [None] + list(range(len(rec["outputs"]))):
            out, grads = run_derivatives(amd, family, gold["inputs"][family], device, only)
            for o, h in zip(out, rec["outputs"]):
                assert same_bits(o, from_hex(h, o.shape))
            want = rec["grads"]["all" if only is None else f"only{only}"]
            assert sorted(grads) == sorted(want)
            for name, g in grads.items():
                _check_gradient(name, g, want[name])


def test_compaction_methods(amd, gold):
    from feos_torch_amd import native

    out = run_compaction(native)
    assert sorted(out) == sorted(gold["compaction"])
    for name, t in out.items():
        assert same_bits(t, from_hex(gold["compaction"][name], t.shape)), name


def test_pure_vle_plan_methods_and_error_names(amd, gold):
    from feos_torch_amd import _lib, native

    inp = with_bad_row(gold["inputs"]["pure"], "pure")
    out = run_plan(native, inp)
    assert sorted(out) == sorted(gold["plan"])
    for name, t in out.items():
        assert same_bits(t, from_hex(gold["plan"][name], t.shape)), name
    # a null required pointer is rejected on the host before any launch; the error names the entry point that was called
    T = torch.tensor(inp["temperature"], dtype=f64, device="cuda")
    for fp64, method, fn in [(False, "run", "pcs_pure_vle"), (True, "run", "pcs_pure_vle_fp64"), (False, "run_fast", "pcs_pure_vle_fast"),
                             (False, "run_retry", "pcs_pure_vle_retry")]:
        plan = native.PureVlePlan(N, "cuda", all_fp64=fp64)
        with pytest.raises(_lib.PcsError) as e:
            getattr(plan, method)(None, T)
        assert str(e.value).startswith(f"{fn} failed"), str(e.value)
