"""GPU: incipient-phase composition of PcSaftMix.bubble_point / dew_point / bubble_temperature / dew_temperature
(incipient_molefracs=True) and pcs_mix_point_jacobian, on the input set of tests/tools/mix_incipient_referee.py (192 parameter
rows x 3 temperature factors per problem).

Bars.  Values: the rho4 bar of tests/test_mix_temperature_gpu.py (max(1e-10, 10 e_p x the cell's d ln rho / d ln p), e_p = the
existing pressure kernel against the oracle per cell).  jac_y: max(10 e, 1e-8), e = the referee's Richardson machinery on p
against the oracle's exact gradient (tests/test_mix_incipient_referee.py: bubble 2.5e-8, dew 9.5e-9), relative to the row's
largest component, every kept row.  jac_p: 1e-8 against the exact gradient (the bar of pcs_mix_jacobian).

"0 < y < 1": three bubble rows of the set have a trace component below 1.1e-16 in the vapour, so the oracle's own y is 1.0 as
a double; there y <= 1 is asked, y < 1 everywhere else.

  1. values  2. jac_y vs referee  3. jac_p vs exact  4. autograd  5. schedule independence  6. round trip  7. graph capture

Measured on the MI355X.  y vs oracle: pressure calls 5.0e-14 (bubble) / 7.2e-14 (dew), temperature calls
2.0e-12 / 5.5e-13.  jac_y vs referee: 1.6e-8 / 5.7e-9 (medians 4.6e-11 / 4.7e-11; bars 2.5e-7 / 9.5e-8).  jac_p vs exact:
1.4e-10 / 4.6e-13.  dy|_p of the temperature calls vs the referee's quotient: 1.8e-8 / 7.4e-9.  Round trip: p 1.8e-13, x 1.3e-13
on the 359 of 566 rows where both calls converge and are stable.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import mix_incipient_referee as ref  # noqa: E402
import mix_temperature_referee as tref  # noqa: E402

pytestmark = pytest.mark.gpu

PROBLEMS = (False, True)
PREFIXES = (1, 63, 64, 65, 127, 128, 129, 385)
f64 = torch.float64
name = lambda dew: "dew" if dew else "bubble"


class Ctx:
    pass


def _d(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _rel(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(a - b) / np.abs(b)


def _model(c, idx, requires_grad=False):
    from feos_torch_amd import PcSaftMix

    P, K = _d(c.P[idx]).requires_grad_(requires_grad), _d(c.K[idx]).requires_grad_(requires_grad)
    return PcSaftMix(P, K), P, K


def _call(eos, dew, temperature_call):
    if temperature_call:
        return eos.dew_temperature if dew else eos.bubble_temperature
    return eos.dew_point if dew else eos.bubble_point


def _args(c, temperature_call):
    """(first argument, mole fractions, start) of a pressure / temperature call on the whole set"""
    if temperature_call:
        return _d(c.p_spec), _d(c.z), _d(0.93 * c.T)
    return _d(c.T), _d(c.z), _d(np.full(c.n, 1e5))


@pytest.fixture(scope="module")
def ctx(oracle, hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from feos_torch_amd import native

    out = {}
    for dew in PROBLEMS:
        c = ref.inputs(oracle, dew)
        g = Ctx()
        g.c, g.dew = c, dew
        g.dev = [_d(v) for v in (c.P, c.K, c.T, c.z, np.full(c.n, 1e5))]
        g.r = native.mix_bubble_dew(*g.dev, dew)
        g.status = g.r["status"].cpu().numpy()
        # value bar: as tests/test_mix_temperature_gpu.py forms it for rho4
        e = tref.per_cell_max(c, _rel(g.r["p"].cpu().numpy(), c.p_spec), c.keep & ~g.status)
        g.bar_rho = np.maximum(1e-10, np.maximum(1e-10, 10.0 * e) * np.maximum(1.0, tref.per_cell_max(c, c.dlnrho_dlnp, c.keep)))
        g.jp, g.jy = native.mix_point_jacobian(g.dev[0], g.dev[1], g.dev[2], g.r["rho4"], dew)
        out[dew] = g
    return out


@pytest.mark.parametrize("temperature_call", (False, True))
@pytest.mark.parametrize("dew", PROBLEMS)
def test_values_against_the_oracle_and_the_default_call(ctx, dew, temperature_call):
    g = ctx[dew]
    c = g.c
    idx = np.arange(c.n)
    a = _args(c, temperature_call)
    base = _call(_model(c, idx)[0], dew, temperature_call)(*a)
    with_y = _call(_model(c, idx)[0], dew, temperature_call)(*a, incipient_molefracs=True)
    assert len(base) == 2 and len(with_y) == 3
    assert torch.equal(base[0], with_y[0]) and torch.equal(base[1], with_y[1])
    base_s = _call(_model(c, idx)[0], dew, temperature_call)(*a, check_stability=True)
    with_s = _call(_model(c, idx)[0], dew, temperature_call)(*a, check_stability=True, incipient_molefracs=True)
    assert len(base_s) == 3 and len(with_s) == 4 and all(torch.equal(u, v) for u, v in zip(base_s, with_s[:3]))
    assert torch.equal(with_s[3], with_y[2]) and torch.equal(base_s[0], base[0])
    y_ok, nans = with_y[2], with_y[1].cpu().numpy()
    assert y_ok.dtype == f64 and y_ok.shape == with_y[0].shape and y_ok.is_cuda
    y = np.full(c.n, np.nan)
    y[~nans] = y_ok.cpu().numpy()
    k = c.keep_y & ~nans
    assert k.sum() >= 0.97 * c.keep_y.sum()
    err = _rel(y, c.y)
    print("%-6s %-11s y vs oracle: %.2e (bar <= %.2e) on %d rows; y in [%.3e, %.17g]" % (
        name(dew), "temperature" if temperature_call else "pressure", err[k].max(), g.bar_rho[k].max(), k.sum(), y[k].min(), y[k].max()))
    assert (err[k] <= g.bar_rho[k]).all(), np.nonzero(k & (err > g.bar_rho))[0]
    assert (y[k] > 0).all() and (y[k] <= 1).all() and (y[k & (c.y < 1)] < 1).all()


@pytest.mark.parametrize("dew", PROBLEMS)
def test_jac_y_against_the_richardson_referee(ctx, dew):
    g = ctx[dew]
    c = g.c
    k = c.keep_y & ~g.status
    err = ref.row_error(g.jy.cpu().numpy(), c.Ry, c.checked)
    print("%-6s jac_y vs referee: max %.2e, median %.2e on %d rows (bar %.2e, e = %.2e)" % (
        name(dew), err[k].max(), np.median(err[k]), k.sum(), c.bar, c.e))
    assert k.sum() >= 0.97 * c.keep_y.sum() and set(np.unique(c.cls[k])) == set(range(tref.N_CLASSES))
    assert (err[k] <= c.bar).all(), (np.nonzero(k & ~(err <= c.bar))[0], err[k].max())


@pytest.mark.parametrize("dew", PROBLEMS)
def test_jac_p_against_the_exact_gradient(ctx, dew):
    g = ctx[dew]
    c = g.c
    k = c.keep & ~g.status
    got = g.jp.cpu().numpy()
    err = np.abs(got - c.grad).max(axis=1) / np.abs(c.grad).max(axis=1)
    print("%-6s jac_p of the new kernel vs exact: %.2e on %d rows" % (name(dew), err[k].max(), k.sum()))
    assert (err[k] < 1e-8).all(), np.nonzero(k & ~(err < 1e-8))[0]


def _dense(n, keep, x):
    out = torch.zeros((n,) + tuple(x.shape[1:]), dtype=f64, device=x.device)
    out[keep] = x
    return out


@pytest.mark.parametrize("dew", PROBLEMS)
def test_autograd_of_the_pressure_calls_is_the_weighted_sum_of_the_blocks(ctx, dew):
    from feos_torch_amd import native

    g = ctx[dew]
    c = g.c
    n = c.n
    T_np = c.T.copy()
    T_np[[3, 130]] = 1e6  # far super-critical: two rows without a solution, whatever the set holds
    r = native.mix_bubble_dew(g.dev[0], g.dev[1], _d(T_np), g.dev[3], g.dev[4], dew)
    keep = ~r["status"]
    assert not keep[3].item() and not keep[130].item()
    jp, jy = native.mix_point_jacobian(g.dev[0][keep], g.dev[1][keep], _d(T_np)[keep], r["rho4"][keep], dew)
    gen = torch.Generator(device="cuda").manual_seed(5)
    wp, wy = (torch.randn(int(keep.sum()), dtype=f64, device="cuda", generator=gen) for _ in range(2))
    for use_p, use_y in ((True, True), (True, False), (False, True)):
        eos, P, K = _model(c, np.arange(n), True)
        T = _d(T_np).requires_grad_(True)
        z, p0 = g.dev[3].clone().requires_grad_(True), g.dev[4].clone().requires_grad_(True)
        p, nans, y = _call(eos, dew, False)(T, z, p0, incipient_molefracs=True)
        assert torch.equal(nans, r["status"])
        loss = 0.0
        if use_p:
            loss = loss + (wp * p).sum()
        if use_y:
            loss = loss + (wy * y).sum()
        gP, gK, gT, gz, gp0 = torch.autograd.grad(loss, (P, K, T, z, p0), allow_unused=True)
        assert gz is None and gp0 is None  # mole fractions and the initial pressure receive no gradient
        want = (wp[:, None] * jp if use_p else 0.0) + (wy[:, None] * jy if use_y else 0.0)
        want = _dense(n, keep, want)
        got = torch.cat((gP.reshape(n, 16), gK, gT[:, None]), dim=1)
        assert (got[~keep] == 0).all().item(), "dropped rows must receive exactly zero"
        assert torch.equal(got, want), (use_p, use_y, float((got - want).abs().max()))
    eos, P, _ = _model(c, np.arange(8), True)
    _, _, y = _call(eos, dew, False)(g.dev[2][:8], g.dev[3][:8], g.dev[4][:8], incipient_molefracs=True)
    (g1,) = torch.autograd.grad(y.sum(), P, create_graph=True)
    assert not g1.requires_grad  # once_differentiable: the gradient carries no graph


@pytest.mark.parametrize("dew", PROBLEMS)
def test_autograd_of_the_temperature_calls_follows_the_line_of_constant_pressure(ctx, dew):
    g = ctx[dew]
    c = g.c
    n = c.n
    p_np = c.p_spec.copy()
    p_np[[5, 50]] = -1.0  # two rows fail at once
    eos, P, K = _model(c, np.arange(n), True)
    ps = _d(p_np).requires_grad_(True)
    z, t0 = _d(c.z).requires_grad_(True), _d(0.93 * c.T).requires_grad_(True)
    T, nans, y = _call(eos, dew, True)(ps, z, t0, incipient_molefracs=True)
    gP, gK, gp, gz, gt0 = torch.autograd.grad(y.sum(), (P, K, ps, z, t0), allow_unused=True)
    assert gz is None and gt0 is None  # mole fractions and the first iterate receive no gradient
    nans = nans.cpu().numpy()
    assert nans[5] and nans[50]
    got = np.concatenate((gP.reshape(n, 16).cpu().numpy(), gK.cpu().numpy(), gp.cpu().numpy()[:, None]), axis=1)
    assert (got[nans] == 0).all(), "dropped rows must receive exactly zero"
    want = ref.quotient(c.Rp, c.Ry)
    checked = c.checked.copy()
    checked[:, 18] = True  # dy/dp_spec is formed on every row
    k = c.keep_y & ~nans
    err = ref.row_error(got, want, checked)
    print("%-6s dy|_p vs the referee's quotient: max %.2e, median %.2e on %d rows (bar %.2e)" % (
        name(dew), err[k].max(), np.median(err[k]), k.sum(), c.bar))
    assert k.sum() >= 0.97 * c.keep_y.sum() - 2
    assert (err[k] <= c.bar).all(), (np.nonzero(k & ~(err <= c.bar))[0], err[k].max())
    # T and y together: the temperature's own gradient is the default call's
    eos2, P2, _ = _model(c, np.arange(n), True)
    T2, _, y2 = _call(eos2, dew, True)(_d(p_np), _d(c.z), _d(0.93 * c.T), incipient_molefracs=True)
    eos3, P3, _ = _model(c, np.arange(n), True)
    T3, _ = _call(eos3, dew, True)(_d(p_np), _d(c.z), _d(0.93 * c.T))
    (a,), (b,) = torch.autograd.grad(T2.sum(), P2), torch.autograd.grad(T3.sum(), P3)
    scale = b.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1e-300)
    assert float(((a - b).abs() / scale).max()) < 1e-8  # two kernels, the same gradient


def _raw(dew, a, rho4, n, want_p=True, want_y=True, workspace=None):
    from feos_torch_amd import _lib

    jp = torch.full((n, 19), float("nan"), dtype=f64, device="cuda") if want_p else None
    jy = torch.full((n, 19), float("nan"), dtype=f64, device="cuda") if want_y else None
    rc = _lib.lib().pcs_mix_point_jacobian(int(dew), _lib.ptr(a[0]), _lib.ptr(a[1]), _lib.ptr(a[2]), _lib.ptr(rho4), n, _lib.ptr(jp),
                                          _lib.ptr(jy), _lib.ptr(workspace), _lib.current_stream_ptr(rho4.device))
    _lib.check(rc, "pcs_mix_point_jacobian")
    torch.cuda.synchronize()
    return jp, jy


@pytest.mark.parametrize("dew", PROBLEMS)
def test_schedule_independence(ctx, dew):
    from feos_torch_amd import native

    g = ctx[dew]
    n = g.c.n
    a, rho4 = g.dev[:3], g.r["rho4"]
    ok = ~g.r["status"]
    assert torch.isfinite(g.jp[ok]).all() and torch.isfinite(g.jy[ok]).all()
    plain = _raw(dew, a, rho4, n)  # no workspace: rows bucketed inside the workgroup
    assert torch.equal(plain[0][ok], g.jp[ok]) and torch.equal(plain[1][ok], g.jy[ok])
    for m in PREFIXES:
        part = native.mix_point_jacobian(a[0][:m].contiguous(), a[1][:m].contiguous(), a[2][:m].contiguous(), rho4[:m].contiguous(), dew)
        assert torch.equal(part[0][ok[:m]], g.jp[:m][ok[:m]]) and torch.equal(part[1][ok[:m]], g.jy[:m][ok[:m]]), m
        part = _raw(dew, [v[:m].contiguous() for v in a], rho4[:m].contiguous(), m)
        assert torch.equal(part[0][ok[:m]], g.jp[:m][ok[:m]]) and torch.equal(part[1][ok[:m]], g.jy[:m][ok[:m]]), m
    only_p = native.mix_point_jacobian(*a, rho4, dew, want_y=False)
    only_y = native.mix_point_jacobian(*a, rho4, dew, want_p=False)
    assert only_p[1] is None and only_y[0] is None
    assert torch.equal(only_p[0][ok], g.jp[ok]) and torch.equal(only_y[1][ok], g.jy[ok])
    with pytest.raises(ValueError):
        native.mix_point_jacobian(*a, rho4, dew, want_p=False, want_y=False)
    # failed rows of a solve (status 1, rho4 zeros) in the batch: the call returns cleanly, the other rows are unchanged
    holed = rho4.clone()
    failed = torch.zeros(n, dtype=torch.bool, device="cuda")
    failed[[0, 7, 64, 200, 383, n - 1]] = True
    holed[failed] = 0.0
    for ws in (True, False):
        got = native.mix_point_jacobian(*a, holed, dew) if ws else _raw(dew, a, holed, n)
        torch.cuda.synchronize()
        m = ok & ~failed
        assert torch.equal(got[0][m], g.jp[m]) and torch.equal(got[1][m], g.jy[m])


def test_round_trip_bubble_then_dew(ctx):
    """bubble_point(T, x) -> (p, y), then dew_point(T, y, p) -> (p, x) again, on the rows where both calls converge and both
    stability flags are True.  The composition travels as ONE double, the mole fraction of component 1: where that is
    1 - 1e-11 the trace component's fraction -- which the dew point hangs on -- has five digits left, and the long-double
    oracle itself then returns to p and x only within 3.1e-5 / 1.8e-5 (set row 135; 1e-8 ... 1e-7 on five more rows).  So
    every row is written with the component that is the minor one in its vapour (by the oracle's y) as component 1: the
    same mixtures, labelled so that the number handed over carries the information.  The oracle's round trip is then
    4e-15 on every row that returns to the same dew branch."""
    g = ctx[False]
    c = g.c
    idx = np.nonzero(c.keep_y)[0]
    swap = c.y[idx] > 0.5
    P_np = np.ascontiguousarray(np.where(swap[:, None, None], c.P[idx][:, ::-1, :], c.P[idx]))
    from feos_torch_amd import PcSaftMix

    eos = PcSaftMix(_d(P_np), _d(c.K[idx]))
    T, x = _d(c.T[idx]), _d(np.where(swap, 1.0 - c.z[idx], c.z[idx]))
    p, nans, stable, y = eos.bubble_point(T, x, _d(np.full(len(idx), 1e5)), check_stability=True, incipient_molefracs=True)
    keep = ~nans
    T1, x1 = T[keep], x[keep]
    assert bool(((y > 0) & (y < 0.51)).all())
    p2, nans2, stable2, x2 = eos.dew_point(T1, y, p, check_stability=True, incipient_molefracs=True)
    both = (~nans2).clone()
    both[~nans2] = stable2
    both &= stable
    sel2 = both[~nans2]
    ep = ((p2[sel2] - p[both]).abs() / p[both]).cpu().numpy()
    ex = ((x2[sel2] - x1[both]).abs() / x1[both]).cpu().numpy()
    bar = g.bar_rho[idx][keep.cpu().numpy()][both.cpu().numpy()]
    print("round trip on %d of %d rows (both converged and stable): p %.2e, x %.2e (bar <= %.2e)" % (
        int(both.sum()), len(idx), ep.max(), ex.max(), bar.max()))
    assert int(both.sum()) >= 0.5 * len(idx)
    assert (ep <= bar).all() and (ex <= bar).all(), (np.nonzero(ep > bar)[0], np.nonzero(ex > bar)[0])


def test_hipgraph_replay_equals_eager(ctx):
    from feos_torch_amd import native

    g = ctx[True]
    a, rho4 = g.dev[:3], g.r["rho4"]
    dev = rho4.device
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        native.mix_point_jacobian(*a, rho4, True)  # warm-up on the capture stream
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        jp, jy = native.mix_point_jacobian(*a, rho4, True)
    jp.fill_(float("nan"))
    jy.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    ok = ~g.r["status"]
    assert torch.equal(jp[ok], g.jp[ok]) and torch.equal(jy[ok], g.jy[ok])
