"""GPU: PcSaftPure.enthalpy_of_vaporization / pcs_pure_enthalpy_of_vaporization(_vjp) on the saturation-line grid
(tests/tools/saturation_grid.py, 256 parameter rows of all four classes x 15 theta = T / T_c from 0.45 to 1.03 = 3,840 rows),
both row orders.  Referees: tests/tools/enthalpy_referee.py (pinned without a GPU by tests/test_enthalpy_referee.py).

  1. values: against the Clausius-Clapeyron value of the long-double oracle; per theta the bar is max(1e-10, 10 x the relative
     discrepancy of the same formula from the oracle's own fp64 run); rho_vl at the grid's density bars;
  2. masks: every row up to SOLVE_ALL_THETA solved, every super-critical row and every bad temperature flagged, failed rows 0;
  3. never wrong: every row reported solved is finite with dh > 0 and rho_V < rho_c < rho_L; dh falls with theta per parameter row;
  4. schedule independence: both orders and the prefixes 1, 63, 64, 65, 257 are bit-identical per row;
  5. consistency: for theta <= 0.99, dh == 1e-6 T dv x column 8 of native.pure_jacobian("vapor_pressure") at the returned
     densities within the bar of 1;
  6. gradients: (a) 48 solved rows (12 per class, theta in {0.6, 0.9, 0.99}) against the exact mpmath gradient, relative to the
     row's largest component, at GRAD_MP_BAR; (b) every row up to theta = 0.99 against four-point central differences of the
     oracle value at relative step 1e-4, per theta at 10 x the disagreement of that difference between steps 1e-4 and 5e-5;
     (c) the vjp with a cotangent == cotangent x the unit-cotangent result, bit for bit;
  7. autograd == the direct vjp call bit for bit with and without dropped rows, zeros in dropped rows, nans == status, the
     model is reduced, CPU tensors in -> CPU tensors out, a second backward is refused.

Measured on the MI355X, identical in both row orders.  Values, error against (a) / the oracle's own fp64 run, per theta: 0.45:
1.5e-15 / 4.8e-14, 0.9: 4.6e-15 / 6.1e-15, 0.99: 7.1e-14 / 9.0e-14, 0.999: 1.5e-12 / 2.4e-12, 0.9995: 4.5e-12 / 7.4e-12, 0.9999:
4.1e-11 / 6.7e-11 (every bar at the 1e-10 floor except 6.6e-10 at 0.9999); rho_V / rho_L within 1.1e-12 up to 0.999 and 2.4e-11
at 0.9999.  Consistency with the vapour-pressure Jacobian: 1.8e-15.  Gradient against mpmath: 7.0e-13; against the central
differences: 3e-10 to 2.6e-8 (theta = 0.99), 0.04 to 0.21 of the bar; no row left out.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import enthalpy_referee as er  # noqa: E402
import saturation_grid as sg  # noqa: E402

pytestmark = pytest.mark.gpu

N_ROWS, SEED = 256, 22
# The highest theta at which every row is solved, in both row orders; above it the share is printed and
# test_solved_rows_are_never_wrong holds.  It is where vapor_pressure solves every row as well
# (tests/test_saturation_line_gpu.py).  Measured on the MI355X: 256/256 at every theta up to 0.999, 211/256 at 0.9995 and 104/256
# at 0.9999, identical in both row orders.
SOLVE_ALL_THETA = 0.999
# 6(a): max(1e-10, 10 x measured); measured on the MI355X 7.0e-13 at theta = 0.6, 7.7e-15 at 0.9, 9.5e-14 at 0.99 (the same
# construction, D3<DN<2>>, reached 3e-14 for the critical point)
GRAD_MP_BAR = 1e-10
MP_THETA = (0.6, 0.9, 0.99)
FD_MAX_THETA = 0.99
ORDERS = ("theta-major", "interleaved")
f64 = torch.float64


class Ctx:
    pass


def _rel(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(a - b) / np.abs(b)


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
    c.dh, c.rv, c.rl, c.st = er.cc_value(oracle, g.P, g.T)
    assert not c.st[c.sub].any() and c.st[~c.sub].all()
    dh64, _, _, st64 = er.cc_value(oracle, g.P, g.T, prec=0, exact=False)
    cond = sg._per_theta(g, _rel(dh64, c.dh), ~c.st & ~st64)
    c.cond = cond
    c.bar = np.array([sg.bar(cond, th) for th in g.theta])
    c.bar_v = np.array([sg.bar(ref["cond"]["rho_v"], th) for th in g.theta])
    c.bar_l = np.array([sg.bar(ref["cond"]["rho_l"], th) for th in g.theta])
    c.perm = sg.interleave(n)
    c.inv = np.argsort(c.perm)
    c.dev = dev = torch.device("cuda")
    c.d = d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    c.runs = {}
    for order in ORDERS:
        idx = c.perm if order == "interleaved" else np.arange(n)
        r = native.pure_enthalpy_of_vaporization(d(g.P[idx]), d(g.T[idx]), want_rho_vl=True)
        back = c.inv if order == "interleaved" else np.arange(n)
        c.runs[order] = {k: v.cpu().numpy()[back] for k, v in r.items()}
    return c


def test_values_against_the_long_double_oracle(ctx):
    g = ctx.g
    for key, r in ctx.runs.items():
        ok = ~r["status"] & ctx.sub
        e, ev, el = _rel(r["dh"], ctx.dh), _rel(r["rho_vl"][:, 0], ctx.rv), _rel(r["rho_vl"][:, 1], ctx.rl)
        for th, sl in sg.theta_slices(g):
            m = ok[sl]
            if th < 1.0 and m.any():
                print("%-12s theta %-7g solved %3d  dh %.2e (oracle fp64 %.2e, bar %.1e, error / bar %.3f)  rho_V %.2e (%.1e)  rho_L %.2e (%.1e)" % (
                    key, th, m.sum(), e[sl][m].max(), ctx.cond[th], ctx.bar[sl][0], e[sl][m].max() / ctx.bar[sl][0],
                    ev[sl][m].max(), ctx.bar_v[sl][0], el[sl][m].max(), ctx.bar_l[sl][0]))
        assert (e[ok] <= ctx.bar[ok]).all(), (key, g.theta[ok][e[ok] > ctx.bar[ok]])
        assert (ev[ok] <= ctx.bar_v[ok]).all(), (key, g.theta[ok][ev[ok] > ctx.bar_v[ok]])
        assert (el[ok] <= ctx.bar_l[ok]).all(), (key, g.theta[ok][el[ok] > ctx.bar_l[ok]])


def test_failure_masks(ctx):
    from feos_torch_amd import native

    g, d = ctx.g, ctx.d
    assert SOLVE_ALL_THETA >= 0.999
    must = g.theta <= SOLVE_ALL_THETA
    for key, r in ctx.runs.items():
        assert not r["status"][must].any(), (key, g.theta[must & r["status"]])
        assert r["status"][~ctx.sub].all(), key
        assert (r["dh"][r["status"]] == 0).all() and (r["rho_vl"][r["status"]] == 0).all()
        for th, sl in sg.theta_slices(g):
            if SOLVE_ALL_THETA < th < 1.0:
                print("%-12s theta %-7g solved %d / %d" % (key, th, (~r["status"][sl]).sum(), sl.stop - sl.start))
    # temperatures without an answer, next to good wave mates
    rows = np.arange(8)  # theta = 0.45 rows
    T = g.T[rows].copy()
    bad = {1: 0.0, 2: -1.0, 3: np.nan, 4: np.inf, 5: -np.inf}
    for i, v in bad.items():
        T[i] = v
    r = native.pure_enthalpy_of_vaporization(d(g.P[rows]), d(T), want_rho_vl=True)
    st, dh, rho = r["status"].cpu().numpy(), r["dh"].cpu().numpy(), r["rho_vl"].cpu().numpy()
    assert st[list(bad)].all() and not st[[0, 6, 7]].any(), st
    assert (dh[list(bad)] == 0).all() and (rho[list(bad)] == 0).all()
    base = ctx.runs["theta-major"]
    for i in (0, 6, 7):  # the mates are unaffected
        assert dh[i].view(np.int64) == base["dh"][i].view(np.int64) and np.array_equal(rho[i].view(np.int64), base["rho_vl"][i].view(np.int64))
    # bad parameters
    P = g.P[rows].copy()
    P[1, 0], P[2, 2], P[3, 1] = -1.0, np.nan, 0.0
    st = native.pure_enthalpy_of_vaporization(d(P), d(g.T[rows]))["status"].cpu().numpy()
    assert st[[1, 2, 3]].all() and not st[[0, 4, 5, 6, 7]].any(), st


def test_solved_rows_are_never_wrong(ctx):
    g = ctx.g
    for key, r in ctx.runs.items():
        ok = ~r["status"]
        dh, rv, rl = r["dh"][ok], r["rho_vl"][ok, 0], r["rho_vl"][ok, 1]
        assert ctx.sub[ok].all(), key  # nothing is solved where no answer exists
        assert np.isfinite(dh).all() and (dh > 0).all(), key
        assert np.isfinite(rv).all() and np.isfinite(rl).all(), key
        assert (rv > 0).all() and (rv < g.rhoc_red[ok]).all() and (g.rhoc_red[ok] < rl).all(), key
        # per parameter row: dh falls with theta over the solved rows
        k = len(sg.THETA)
        table = np.where(r["status"], np.nan, r["dh"]).reshape(k, N_ROWS)
        for i in range(N_ROWS):
            col = table[:, i][np.isfinite(table[:, i])]
            assert (np.diff(col) < 0).all(), (key, i)


def test_schedule_independence(ctx):
    from feos_torch_amd import native

    a, b = ctx.runs["theta-major"], ctx.runs["interleaved"]
    for k in ("dh", "rho_vl", "status"):
        v = np.uint8 if k == "status" else np.int64
        assert np.array_equal(a[k].view(v), b[k].view(v)), k
    for m in sg.PREFIXES:
        idx = ctx.perm[:m]
        r = native.pure_enthalpy_of_vaporization(ctx.d(ctx.g.P[idx]), ctx.d(ctx.g.T[idx]), want_rho_vl=True)
        assert np.array_equal(r["status"].cpu().numpy(), b["status"][idx]), m
        assert np.array_equal(r["dh"].cpu().numpy().view(np.int64), b["dh"][idx].view(np.int64)), m
        assert np.array_equal(r["rho_vl"].cpu().numpy().view(np.int64), b["rho_vl"][idx].view(np.int64)), m
    # the gradient kernel too: prefixes of a 512-row call alone (partial workgroups: idle lanes repeat the last row)
    idx = ctx.perm[~b["status"][ctx.perm]][:512]
    full = _vjp(ctx, ctx.g.P[idx], ctx.g.T[idx], b["rho_vl"][idx])
    assert len(idx) == 512 and torch.isfinite(full).all().item()
    for m in sg.PREFIXES:
        part = _vjp(ctx, ctx.g.P[idx[:m]], ctx.g.T[idx[:m]], b["rho_vl"][idx[:m]])
        assert torch.equal(part.view(torch.int64), full[:m].view(torch.int64)), m
    # the value does not depend on whether the densities are requested
    r = native.pure_enthalpy_of_vaporization(ctx.d(ctx.g.P), ctx.d(ctx.g.T))
    assert "rho_vl" not in r and np.array_equal(r["dh"].cpu().numpy().view(np.int64), a["dh"].view(np.int64))


def test_consistency_with_the_vapour_pressure_jacobian(ctx):
    from feos_torch_amd import native

    g, d = ctx.g, ctx.d
    r = ctx.runs["theta-major"]
    rows = g.theta <= 0.99
    assert not r["status"][rows].any()
    jac = native.pure_jacobian("vapor_pressure", d(g.P[rows]), d(g.T[rows]), None, d(r["rho_vl"][rows])).cpu().numpy()
    rv, rl = r["rho_vl"][rows, 0], r["rho_vl"][rows, 1]
    cc = 1e-6 * g.T[rows] * (1.0 / rv - 1.0 / rl) * er.RHO_UNIT * jac[:, 8]
    err = _rel(r["dh"][rows], cc)
    print("dh vs 1e-6 T dv x Jacobian column 8: max rel %.2e, max error / bar %.3f" % (err.max(), (err / ctx.bar[rows]).max()))
    assert (err <= ctx.bar[rows]).all()


def _vjp(ctx, P, T, rho, gout=None):
    from feos_torch_amd import native

    gout = torch.ones(len(T), dtype=f64, device=ctx.dev) if gout is None else gout
    gp, gt = native.pure_enthalpy_of_vaporization_vjp(ctx.d(P), ctx.d(T), ctx.d(rho), gout)
    return torch.cat([gp, gt[:, None]], dim=1)


def test_gradient_against_mpmath(ctx):
    g = ctx.g
    r = ctx.runs["theta-major"]
    cls = sg.classes(g.P[:N_ROWS])
    rows = []
    for th in MP_THETA:
        k = sg.THETA.index(th)
        for c in range(4):
            rows += [k * N_ROWS + i for i in np.nonzero(cls == c)[0][:4]]
    rows = np.array(rows)
    assert len(rows) == 48 and not r["status"][rows].any()
    G = _vjp(ctx, g.P[rows], g.T[rows], r["rho_vl"][rows]).cpu().numpy()
    worst = {th: 0.0 for th in MP_THETA}
    for j, i in enumerate(rows):
        E = er.mp_gradient(g.P[i], g.T[i], r["rho_vl"][i, 0], r["rho_vl"][i, 1])
        worst[g.theta[i]] = max(worst[g.theta[i]], np.abs(G[j] - E).max() / np.abs(E).max())
    print("gradient vs mpmath, max error / largest component per theta: " + ", ".join("%g: %.2e" % kv for kv in worst.items()))
    assert max(worst.values()) <= GRAD_MP_BAR


def test_gradient_against_central_differences_of_the_oracle(ctx):
    g, orc = ctx.g, ctx.orc
    r = ctx.runs["theta-major"]
    rows = g.theta <= FD_MAX_THETA
    assert not r["status"][rows].any()
    P, T = np.ascontiguousarray(g.P[rows]), np.ascontiguousarray(g.T[rows])
    G = _vjp(ctx, P, T, r["rho_vl"][rows]).cpu().numpy()
    fd, fd2 = er.cc_central_difference(orc, P, T, 1e-4), er.cc_central_difference(orc, P, T, 5e-5)
    usable = np.isfinite(fd).all(axis=1) & np.isfinite(fd2).all(axis=1)
    assert (~usable).sum() <= 0.01 * len(T), (~usable).sum()
    scale = np.abs(fd).max(axis=1)
    with np.errstate(invalid="ignore"):
        err, own = np.abs(G - fd).max(axis=1) / scale, np.abs(fd2 - fd).max(axis=1) / scale
    th_rows = g.theta[rows]
    for th in sg.SUB:
        m = (th_rows == th) & usable
        if not m.any():
            continue
        bar = 10.0 * own[m].max()
        print("theta %-7g vjp vs central differences: max %.2e, steps 1e-4 vs 5e-5 %.2e, bar %.1e, left out %d" % (
            th, err[m].max(), own[m].max(), bar, ((th_rows == th) & ~usable).sum()))
        assert err[m].max() <= bar, th
    assert np.isfinite(G).all()


def test_vjp_is_the_cotangent_times_the_unit_result(ctx):
    g = ctx.g
    r = ctx.runs["theta-major"]
    ok = ~r["status"]
    unit = _vjp(ctx, g.P[ok], g.T[ok], r["rho_vl"][ok])
    gout = ctx.d(np.random.default_rng(3).uniform(-2.0, 2.0, int(ok.sum())))
    got = _vjp(ctx, g.P[ok], g.T[ok], r["rho_vl"][ok], gout)
    assert torch.isfinite(unit).all().item()
    assert torch.equal(got.view(torch.int64), (gout[:, None] * unit).view(torch.int64))


def test_autograd_equals_the_direct_calls(ctx):
    from feos_torch_amd import PcSaftPure, native

    g, d = ctx.g, ctx.d
    cases = {"every row solved": g.theta <= 0.9, "rows dropped": np.ones(ctx.n, dtype=bool)}
    for name, rows in cases.items():
        P = d(g.P[rows]).requires_grad_(True)
        T = d(g.T[rows]).requires_grad_(True)
        eos = PcSaftPure(P)
        nans, dh = eos.enthalpy_of_vaporization(T)
        direct = native.pure_enthalpy_of_vaporization(P.detach(), T.detach(), want_rho_vl=True)
        st = direct["status"].cpu().numpy()
        assert np.array_equal(nans.cpu().numpy(), st) and np.array_equal(st, ctx.runs["theta-major"]["status"][rows]), name
        assert nans.any().item() == (name == "rows dropped")
        assert eos.parameters.shape == (int((~st).sum()), 8)  # the model is reduced by the call
        keep = torch.from_numpy(~st).to(ctx.dev)
        assert torch.equal(dh.detach(), direct["dh"][keep])
        w = torch.linspace(0.5, 1.5, dh.shape[0], dtype=f64, device=ctx.dev)
        (w * dh).sum().backward()
        gp, gt = native.pure_enthalpy_of_vaporization_vjp(P.detach()[keep], T.detach()[keep], direct["rho_vl"][keep], w)
        assert torch.equal(P.grad[keep].view(torch.int64), gp.view(torch.int64)), name
        assert torch.equal(T.grad[keep].view(torch.int64), gt.view(torch.int64)), name
        assert (P.grad[~keep] == 0).all().item() and (T.grad[~keep] == 0).all().item(), name
        assert torch.isfinite(P.grad).all().item() and torch.isfinite(T.grad).all().item(), name
    # only one of the two inputs asks for a gradient
    P = d(g.P[:64]).requires_grad_(True)
    nans, dh = PcSaftPure(P).enthalpy_of_vaporization(d(g.T[:64]))
    dh.sum().backward()
    assert P.grad.shape == (64, 8) and not nans.any().item()


def test_shell_conventions(ctx):
    from feos_torch_amd import PcSaftPure

    g = ctx.g
    base = ctx.runs["theta-major"]
    rows = np.concatenate([np.arange(0, 70), np.arange(ctx.n - 30, ctx.n)])  # 70 rows at theta = 0.45, 30 super-critical
    par = torch.from_numpy(np.ascontiguousarray(g.P[rows])).requires_grad_(True)
    eos = PcSaftPure(par)
    nans, dh = eos.enthalpy_of_vaporization(torch.from_numpy(np.ascontiguousarray(g.T[rows])))
    assert not nans.is_cuda and not dh.is_cuda and nans.dtype == torch.bool and nans.shape == (100,) and dh.shape == (70,)
    assert np.array_equal(nans.numpy(), base["status"][rows]) and np.array_equal(dh.detach().numpy(), base["dh"][rows][:70])
    assert eos.parameters.shape == (70, 8) and np.array_equal(eos.parameters, g.P[rows][:70])
    (gr,) = torch.autograd.grad(dh.sum(), par, create_graph=True)
    assert not gr.is_cuda and gr.shape == (100, 8) and (gr[70:] == 0).all().item()
    assert not gr.requires_grad  # once_differentiable: the gradient carries no graph, so a second backward raises
    with pytest.raises(RuntimeError, match="once_differentiable|differentiate twice|does not require grad"):
        gr.sum().backward()
