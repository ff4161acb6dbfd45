"""GPU: PcSaftPure.boiling_temperature / pcs_pure_boiling_temperature and the Jacobian selector 3 on the saturation-line grid
(tests/tools/saturation_grid.py, 256 parameter rows of all four classes x 15 theta = T / T_c from 0.45 to 1.03 = 3,840 rows).

Inputs: on the sub-critical rows p_spec = the long-double oracle's p_sat, so the exact answer is the grid temperature; on the
super-critical rows p_spec = 1.05 p_c (no answer; these rows are also wave mates).  Both row orders, three starts: none,
0.5 T_c and 0.98 T_c on every row.

  1. values: |T - T_grid| / T_grid <= max(1e-10, 10 x the oracle's own fp64-vs-long-double discrepancy of p_sat at that theta)
     (T inherits at most the relative error of p: d ln p / d ln T > 1), the densities at their own bars;
  2. masks: every row up to SOLVE_ALL_THETA solved, every super-critical row and every bad pressure flagged;
  3. never wrong: every row reported solved, anywhere, is finite, 0 < T < T_c, rho_V < rho_c < rho_L, and the long-double
     oracle's p_sat at the returned T is p_spec within max(15, d ln p / d ln T) x the bar of 1;
  4. schedule independence: both orders and the prefixes 1, 63, 64, 65, 257 are bit-identical per row;
  5. start independence: same mask up to SOLVE_ALL_THETA, T within twice the bar of 1;
  6. gradients: the Jacobian (selector 3) against the quotient of the oracle's exact vapour-pressure gradient at the same state,
     relative to the row's largest component, at max(1e-12, 10 x the same quotient from the oracle's fp64 gradient against its
     long-double one); vjp == gout x Jacobian bit for bit; both autograd routes == the direct calls; dT/dp > 0; no gradient
     to initial_temperature;
  7. round trip: PcSaftPure.vapor_pressure(T_b) == p_spec within 15 x 1e-10, none flagged up to min(SOLVE_ALL_THETA, 0.999);
  8. shell conventions: the model is reduced, CPU tensors in -> CPU tensors out, create_graph=True is refused.

Measured on the MI355X.  6(a), error of the Jacobian / the oracle's own fp64-vs-long-double quotient, relative to the row's
largest component, per theta (all bars at the 1e-12 floor): 0.99: 8.2e-15 / 8.7e-15, 0.995: 1.4e-14 / 1.9e-14, 0.999: 3.3e-14 /
3.4e-14, 0.9995: 3.4e-14 / 4.2e-14, 0.9999: 1.0e-13 / 9.5e-14; below 0.99 smaller.  Values: T within 1.7e-13 of the grid
temperature everywhere, rho_V within 9.9e-12 and rho_L within 8.9e-12 up to 0.9995 (4.3e-11 / 3.0e-11 at 0.9999); the oracle's
p_sat at the returned T within 1.1e-12 of p_spec; the three starts agree on T within 1.7e-13.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import saturation_grid as sg  # noqa: E402

pytestmark = pytest.mark.gpu

N_ROWS, SEED = 256, 22
P_BAR = 1e-10
# The highest theta at which every row is solved (both orders, all three starts, kernel call and PcSaftPure); above it the
# share is printed and test_solved_rows_are_never_wrong holds.  Measured on the MI355X, identical in both row orders:
# 256/256 at every theta up to 0.9995 with all three starts; at 0.9999 229/256 without a start, 256/256 from 0.5 T_c and
# 255/256 from 0.98 T_c.
SOLVE_ALL_THETA = 0.9995
# vapor_pressure itself answers every row only up to here (tests/test_saturation_line_gpu.py::SOLVE_ALL_THETA; 77 % of the
# rows at 0.9995): the round trip asks it to flag none up to the lower of the two
VP_SOLVE_ALL_THETA = 0.999
STARTS = ("none", "0.5Tc", "0.98Tc")
ORDERS = ("theta-major", "interleaved")
f64 = torch.float64


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(oracle, hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from feos_torch_amd import native

    c = Ctx()
    c.orc = oracle
    c.g = g = sg.grid(n_rows=N_ROWS, seed=SEED, orc=oracle)
    c.ref = ref = sg.reference(n_rows=N_ROWS, seed=SEED, orc=oracle)
    c.n = n = len(g.T)
    c.sub = sg.sub_mask(g)
    assert not ref["ld"]["st_p"][c.sub].any() and not ref["ld"]["st_vle"][c.sub].any()
    c.p = np.where(c.sub, ref["ld"]["p_sat"], 1.05 * g.pc)
    c.perm = sg.interleave(n)
    c.inv = np.argsort(c.perm)
    c.dev = dev = torch.device("cuda")
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    c.P, c.pd = d(g.P), d(c.p)
    c.t0 = {"none": None, "0.5Tc": 0.5 * g.Tc, "0.98Tc": 0.98 * g.Tc}
    c.bar_T = np.array([sg.bar(ref["cond"]["p_sat"], th) for th in g.theta])
    c.bar_v = np.array([sg.bar(ref["cond"]["rho_v"], th) for th in g.theta])
    c.bar_l = np.array([sg.bar(ref["cond"]["rho_l"], th) for th in g.theta])
    with np.errstate(invalid="ignore", divide="ignore"):
        slope = ref["grad"]["vapor_pressure"][:, 8] * g.T / ref["ld"]["p_sat"]
    c.slope_factor = max(15.0, float(np.nanmax(slope[c.sub])))
    # every (order, start) once: results as numpy arrays in theta-major order
    c.runs = {}
    for order in ORDERS:
        idx = c.perm if order == "interleaved" else np.arange(n)
        for start in STARTS:
            t0 = c.t0[start]
            r = native.pure_boiling_temperature(d(g.P[idx]), d(c.p[idx]), None if t0 is None else d(t0[idx]), want_iters=True)
            back = c.inv if order == "interleaved" else np.arange(n)
            c.runs[order, start] = {k: v.cpu().numpy()[back] for k, v in r.items()}
    return c


def _rel(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(a - b) / np.abs(b)


def test_values_against_the_long_double_oracle(ctx):
    g, ld = ctx.g, ctx.ref["ld"]
    for key, r in ctx.runs.items():
        ok = ~r["status"] & ctx.sub
        eT, ev, el = _rel(r["t"], g.T), _rel(r["rho_vl"][:, 0], ld["rho_v"]), _rel(r["rho_vl"][:, 1], ld["rho_l"])
        for th, sl in sg.theta_slices(g):
            m = ok[sl]
            if th < 1.0 and m.any():
                print("%-24s theta %-7g solved %3d  T %.2e (bar %.1e)  rho_V %.2e (%.1e)  rho_L %.2e (%.1e)  trials <= %d" % (
                    key, th, m.sum(), eT[sl][m].max(), ctx.bar_T[sl][0], ev[sl][m].max(), ctx.bar_v[sl][0], el[sl][m].max(),
                    ctx.bar_l[sl][0], r["iters"][sl][m].max()))
        assert (eT[ok] <= ctx.bar_T[ok]).all(), (key, g.theta[ok][eT[ok] > ctx.bar_T[ok]])
        assert (ev[ok] <= ctx.bar_v[ok]).all(), (key, g.theta[ok][ev[ok] > ctx.bar_v[ok]])
        assert (el[ok] <= ctx.bar_l[ok]).all(), (key, g.theta[ok][el[ok] > ctx.bar_l[ok]])


def test_failure_masks(ctx):
    from feos_torch_amd import PcSaftPure, native

    g = ctx.g
    must = g.theta <= SOLVE_ALL_THETA
    for key, r in ctx.runs.items():
        assert not r["status"][must].any(), (key, g.theta[must & r["status"]])
        assert r["status"][~ctx.sub].all(), key
        assert (r["t"][r["status"]] == 0).all() and (r["rho_vl"][r["status"]] == 0).all() and (r["iters"][r["status"]] == -1).all()
        for th, sl in sg.theta_slices(g):
            if SOLVE_ALL_THETA < th < 1.0 or th in (0.995, 0.999, 0.9995, 0.9999):
                print("%-24s theta %-7g solved %d / %d" % (key, th, (~r["status"][sl]).sum(), sl.stop - sl.start))
    # the same through the model class, both orders and all three starts: the kernel's mask and values
    d = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(ctx.dev)
    for order in ORDERS:
        idx = ctx.perm if order == "interleaved" else np.arange(ctx.n)
        for start in STARTS:
            t0 = ctx.t0[start]
            nans, T = PcSaftPure(d(g.P[idx])).boiling_temperature(d(ctx.p[idx]), d(None if t0 is None else t0[idx]))
            r = ctx.runs[order, start]
            assert np.array_equal(nans.cpu().numpy(), r["status"][idx]), (order, start)
            assert np.array_equal(T.cpu().numpy(), r["t"][idx][~r["status"][idx]]), (order, start)
    # pressures without an answer, next to good wave mates
    k = 8
    rows = np.arange(k)  # theta = 0.45 rows
    p = ctx.p[rows].copy()
    bad = {1: 2.0 * g.pc[1], 2: 0.0, 3: -1.0, 4: np.nan, 5: np.inf, 6: -np.inf}
    for i, v in bad.items():
        p[i] = v
    r = native.pure_boiling_temperature(d(g.P[rows]), d(p))
    st = r["status"].cpu().numpy()
    assert st[list(bad)].all() and not st[[0, 7]].any(), st
    assert (r["t"].cpu().numpy()[list(bad)] == 0).all()


def test_solved_rows_are_never_wrong(ctx):
    g, orc = ctx.g, ctx.orc
    for key, r in ctx.runs.items():
        ok = ~r["status"]
        T, rv, rl = r["t"][ok], r["rho_vl"][ok, 0], r["rho_vl"][ok, 1]
        assert np.isfinite(T).all() and (T > 0).all() and (T < g.Tc[ok]).all(), key
        assert (rv > 0).all() and (rv < g.rhoc_red[ok]).all() and (g.rhoc_red[ok] < rl).all(), key
        assert ctx.sub[ok].all(), key  # nothing is solved where no answer exists
        p, st = orc.pure_vapor_pressure(np.ascontiguousarray(g.P[ok]), np.ascontiguousarray(T), prec=1)
        assert not st.any(), (key, g.theta[ok][st])
        err = _rel(p, ctx.p[ok])
        print("%-24s oracle p_sat(T_returned) vs p_spec: max %.2e, max / allowed %.3f" % (
            key, err.max(), (err / (ctx.slope_factor * ctx.bar_T[ok])).max()))
        assert (err <= ctx.slope_factor * ctx.bar_T[ok]).all(), (key, g.theta[ok][err > ctx.slope_factor * ctx.bar_T[ok]])


def test_schedule_independence(ctx):
    from feos_torch_amd import native

    for start in STARTS:
        a, b = ctx.runs["theta-major", start], ctx.runs["interleaved", start]
        for k in ("t", "rho_vl", "status"):
            assert np.array_equal(a[k].view(np.uint8 if k == "status" else np.int64), b[k].view(np.uint8 if k == "status" else np.int64)), (start, k)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(ctx.dev)
    full = ctx.runs["interleaved", "none"]
    for m in sg.PREFIXES:
        idx = ctx.perm[:m]
        r = native.pure_boiling_temperature(d(ctx.g.P[idx]), d(ctx.p[idx]))
        assert np.array_equal(r["status"].cpu().numpy(), full["status"][idx]), m
        assert np.array_equal(r["t"].cpu().numpy().view(np.int64), full["t"][idx].view(np.int64)), m
        assert np.array_equal(r["rho_vl"].cpu().numpy().view(np.int64), full["rho_vl"][idx].view(np.int64)), m


def test_start_independence(ctx):
    g = ctx.g
    must = g.theta <= SOLVE_ALL_THETA
    base = ctx.runs["theta-major", "none"]
    for start in STARTS[1:]:
        r = ctx.runs["theta-major", start]
        assert np.array_equal(r["status"][must], base["status"][must]), start
        both = ~r["status"] & ~base["status"]
        err = _rel(r["t"][both], base["t"][both])
        print("start %-7s vs none: max rel difference of T %.2e, max / allowed %.3f" % (start, err.max(), (err / (2 * ctx.bar_T[both])).max()))
        assert (err <= 2.0 * ctx.bar_T[both]).all(), start


def _quotient(g0):
    """[n,10] boiling-temperature Jacobian from the vapour-pressure gradient g0 [n,10]"""
    out = np.zeros_like(g0)
    out[:, :8] = -g0[:, :8] / g0[:, 8:9]
    out[:, 9] = 1.0 / g0[:, 8]
    return out


def test_jacobian_and_vjp_against_the_exact_gradient(ctx):
    from feos_torch_amd import native

    g, orc = ctx.g, ctx.orc
    r = ctx.runs["theta-major", "none"]
    ok = ~r["status"]
    P, T = np.ascontiguousarray(g.P[ok]), np.ascontiguousarray(r["t"][ok])
    rv, rl = np.ascontiguousarray(r["rho_vl"][ok, 0]), np.ascontiguousarray(r["rho_vl"][ok, 1])
    _, exact = orc.pure_property_grad("vapor_pressure", P, T, None, rv, rl, exact=True)
    _, fp64 = orc.pure_property_grad("vapor_pressure", P, T, None, rv, rl, exact=False)
    want, own = _quotient(exact), _quotient(fp64)
    scale = np.abs(want).max(axis=1)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(ctx.dev)
    Pd, Td, rho = d(P), d(T), d(r["rho_vl"][ok])
    jac_t = native.pure_jacobian("boiling_temperature", Pd, Td, None, rho)
    jac = jac_t.cpu().numpy()
    err = np.abs(jac - want).max(axis=1) / scale
    ref_err = np.abs(own - want).max(axis=1) / scale
    th_ok = g.theta[ok]
    for th in sg.SUB:
        m = th_ok == th
        if not m.any():
            continue
        bar = max(1e-12, 10.0 * ref_err[m].max())
        print("theta %-7g Jacobian vs exact quotient: max %.2e, oracle fp64 %.2e, bar %.1e" % (th, err[m].max(), ref_err[m].max(), bar))
        assert err[m].max() <= bar, th
    assert (jac[:, 8] == 0).all() and (jac[:, 9] > 0).all()  # (d): dT/dp = 1 / (dp_sat/dT) > 0
    # (b) the vector-Jacobian form: gout x Jacobian, bit for bit
    gout = d(np.random.default_rng(3).uniform(0.5, 2.0, len(T)))
    gp, gt, gpr = native.pure_jacobian_vjp("boiling_temperature", Pd, Td, None, rho, gout)
    assert torch.equal(gp.view(torch.int64), (gout[:, None] * jac_t[:, :8]).view(torch.int64))
    assert torch.equal(gpr.view(torch.int64), (gout * jac_t[:, 9]).view(torch.int64))
    assert (gt == 0).all().item()


def test_autograd_routes_equal_the_direct_calls(ctx):
    from feos_torch_amd import PcSaftPure, native

    g = ctx.g
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(ctx.dev)
    cases = {"every row solved (vjp kernel)": g.theta <= 0.9, "rows dropped (Jacobian + scatter)": np.ones(ctx.n, dtype=bool)}
    for name, rows in cases.items():
        P = d(g.P[rows]).requires_grad_(True)
        p = d(ctx.p[rows]).requires_grad_(True)
        t0 = d(0.7 * g.Tc[rows]).requires_grad_(True)
        eos = PcSaftPure(P)
        nans, T = eos.boiling_temperature(p, t0)
        direct = native.pure_boiling_temperature(P.detach(), p.detach(), t0.detach())
        st = direct["status"].cpu().numpy()
        assert np.array_equal(nans.cpu().numpy(), st), name
        assert not st[g.theta[rows] <= SOLVE_ALL_THETA].any() and st[~ctx.sub[rows]].all(), name
        assert nans.any().item() == (name != "every row solved (vjp kernel)")
        assert eos.parameters.shape == (int((~st).sum()), 8)  # the model is reduced by the call
        w = torch.linspace(0.5, 1.5, T.shape[0], dtype=f64, device=ctx.dev)
        (w * T).sum().backward()
        assert t0.grad is None  # (e): the first iterate receives no gradient
        keep = torch.from_numpy(~st).to(ctx.dev)
        r = native.pure_boiling_temperature(P.detach()[keep], p.detach()[keep], t0.detach()[keep])
        assert torch.equal(r["t"], T.detach()) and torch.equal(r["t"], direct["t"][keep])
        gp, _, gpr = native.pure_jacobian_vjp("boiling_temperature", P.detach()[keep], r["t"], None, r["rho_vl"], w)
        assert torch.equal(P.grad[keep].view(torch.int64), gp.view(torch.int64)), name
        assert torch.equal(p.grad[keep].view(torch.int64), gpr.view(torch.int64)), name
        assert (P.grad[~keep] == 0).all().item() and (p.grad[~keep] == 0).all().item(), name
        assert (p.grad[keep] > 0).all().item(), name


def test_round_trip_and_shell_conventions(ctx):
    from feos_torch_amd import PcSaftPure

    g = ctx.g
    base = ctx.runs["theta-major", "none"]
    ok = ~base["status"]
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(ctx.dev)
    nans, p = PcSaftPure(d(g.P[ok])).vapor_pressure(d(base["t"][ok]))
    nans = nans.cpu().numpy()
    assert not nans[g.theta[ok] <= min(SOLVE_ALL_THETA, VP_SOLVE_ALL_THETA)].any()
    err = _rel(p.cpu().numpy(), ctx.p[ok][~nans])
    print("vapor_pressure(T_b) vs p_spec: max %.2e; flagged above SOLVE_ALL_THETA: %d" % (err.max(), nans.sum()))
    assert err.max() <= 15.0 * P_BAR
    # CPU tensors in, CPU tensors out, the model reduced to the solved rows
    rows = np.concatenate([np.arange(0, 70), np.arange(ctx.n - 30, ctx.n)])  # 70 rows at theta = 0.45, 30 super-critical
    par = torch.from_numpy(np.ascontiguousarray(g.P[rows])).requires_grad_(True)
    eos = PcSaftPure(par)
    nans, T = eos.boiling_temperature(torch.from_numpy(np.ascontiguousarray(ctx.p[rows])))
    assert not nans.is_cuda and not T.is_cuda and nans.dtype == torch.bool and nans.shape == (100,) and T.shape == (70,)
    assert np.array_equal(nans.numpy(), base["status"][rows]) and np.array_equal(T.detach().numpy(), base["t"][rows][:70])
    assert eos.parameters.shape == (70, 8) and np.array_equal(eos.parameters, g.P[rows][:70])
    (gr,) = torch.autograd.grad(T.sum(), par, create_graph=True)
    assert not gr.requires_grad  # once_differentiable: the gradient carries no graph, so a second backward raises
    with pytest.raises(RuntimeError, match="once_differentiable|differentiate twice|does not require grad"):
        gr.sum().backward()
