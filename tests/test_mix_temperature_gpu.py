"""GPU: PcSaftMix.bubble_temperature / dew_temperature and pcs_mix_bubble_dew_temperature on the input set of
tests/tools/mix_temperature_referee.py: 192 parameter rows (6 association classes x 32) x 3 temperature factors = 576 rows per
problem, p_spec = the long-double oracle's pressure at T_grid (the exact answer is T_grid), three starts on every row
(T_grid, 0.93 T_grid, 1.07 T_grid), two row orders (as built, interleaved).

Bars.  e = the largest relative deviation of the EXISTING native.mix_bubble_dew pressure at T_grid from the oracle's, per
(class, factor, problem) cell; bar = max(1e-10, 10 e) (T inherits at most the relative error of p, d ln p / d ln T > 1; factor
10 as tests/test_boiling_gpu.py).  rho4: max(bar x the cell's largest d ln rho / d ln p along the line (>= 1), 1e-10 of
tests/test_mix_gpu.py).  Gradients: relative to the row's largest component, max(1e-10, 10 x the same quotient formed from
the oracle's fp64 gradient against its exact one).

  1. values  2. masks (every kept row solved from all starts; bad p_spec / t_init flagged, wave mates bit-identical)
  3. never wrong (the oracle's pressure at the returned T is p_spec within max(15, d ln p / d ln T) x bar)
  4. schedule independence (orders, prefixes, with / without workspace: bit-identical)   5. start independence (2 x bar)
  6. gradients   7. round trip through bubble_point / dew_point (15 x bar)   8. shell conventions

Measured on the MI355X (both row orders identical).  e, largest cell: bubble 1.2e-13, dew 4.2e-13, so every bar_T is at the
1e-10 floor; bar_rho <= 6.8e-10 (bubble) / 4.3e-10 (dew).  Rows kept: bubble 566 of 576, dew 576 of 576; all solved from all
three starts.  |T / T_grid - 1|: 1.5e-16 from T_grid (1 trial), bubble 1.1e-13 / 1.0e-13 and dew 1.2e-13 / 8.6e-14 from
0.93 / 1.07 T_grid (median 6 trials with the confirming one; max 6 bubble, 11 dew).  rho4: bubble 5.2e-12, dew 1.1e-12.
Oracle p(T) against p_spec: <= 1.0e-12.  The three starts agree on T within 1.2e-13.  Gradient, relative to the row's largest
component: bubble 1.6e-10 (the oracle's fp64 quotient against its exact one: up to 6.6e-6 in a cell), dew 9.1e-13 (2.4e-8);
dT/dp within 9.1e-13.  Round trip through bubble_point / dew_point: 1.0e-12.  Without the confirming cold trial
(csrc/mix_temperature.hpp) five dew rows started at 0.93 T_grid end on the other dew branch, up to 7 % from T_grid.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import mix_temperature_referee as ref  # noqa: E402

pytestmark = pytest.mark.gpu

PROBLEMS = (False, True)
ORDERS = ("as built", "interleaved")
PREFIXES = (1, 63, 64, 65, 127, 128, 129, 257)
f64 = torch.float64
name = lambda dew: "dew" if dew else "bubble"


class Ctx:
    pass


def _d(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _rel(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(a - b) / np.abs(b)


def _run(c, dew, idx, start, **kw):
    from feos_torch_amd import native

    r = native.mix_bubble_dew_temperature(_d(c.P[idx]), _d(c.K[idx]), _d(c.p_spec[idx]), _d(c.z[idx]), _d(start * c.T[idx]), dew,
                                          want_iters=True, **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


@pytest.fixture(scope="module")
def ctx(oracle, hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from feos_torch_amd import native

    out = {}
    for dew in PROBLEMS:
        c = ref.inputs(oracle, dew)
        k = c.keep
        # e: the parent's pressure kernel against the oracle at T_grid, per cell
        r = native.mix_bubble_dew(_d(c.P), _d(c.K), _d(c.T), _d(c.z), _d(np.full(c.n, 1e5)), dew)
        p_gpu, st = r["p"].cpu().numpy(), r["status"].cpu().numpy()
        g = Ctx()
        g.c, g.dew = c, dew
        g.e = ref.per_cell_max(c, _rel(p_gpu, c.p_spec), k & ~st)
        g.bar = np.maximum(1e-10, 10.0 * g.e)
        g.bar_rho = np.maximum(1e-10, g.bar * np.maximum(1.0, ref.per_cell_max(c, c.dlnrho_dlnp, k)))
        q, q64 = ref.quotient(c.grad), ref.quotient(c.grad64)
        with np.errstate(invalid="ignore", divide="ignore"):
            eg = np.abs(q64 - q).max(axis=1) / np.abs(q).max(axis=1)
        g.e_grad = ref.per_cell_max(c, eg, k)
        g.bar_grad = np.maximum(1e-10, 10.0 * g.e_grad)
        g.perm = ref.interleave(c.n)
        g.inv = np.argsort(g.perm)
        g.runs = {}
        for order in ORDERS:
            idx = g.perm if order == "interleaved" else np.arange(c.n)
            back = g.inv if order == "interleaved" else np.arange(c.n)
            for s in ref.STARTS:
                g.runs[order, s] = {key: v[back] for key, v in _run(c, dew, idx, s).items()}
        out[dew] = g
    return out


@pytest.mark.parametrize("dew", PROBLEMS)
def test_values_against_the_long_double_oracle(ctx, dew):
    g = ctx[dew]
    c, k = g.c, g.c.keep
    print("%s: e = %.2e (largest cell), bar_T <= %.2e, bar_rho <= %.2e" % (name(dew), g.e.max(), g.bar.max(), g.bar_rho.max()))
    for key, r in g.runs.items():
        ok = k & ~r["status"]
        eT = _rel(r["t"], c.T)
        er = _rel(r["rho4"], c.rho4).max(axis=1)
        print("%-7s %-12s start %.2f  solved %3d / %3d kept  T %.2e  rho4 %.2e  trials: median %d, max %d" % (
            name(dew), key[0], key[1], ok.sum(), k.sum(), eT[ok].max(), er[ok].max(), np.median(r["iters"][ok]), r["iters"][ok].max()))
        assert (eT[ok] <= g.bar[ok]).all(), (key, np.nonzero(ok & (eT > g.bar))[0], eT[ok].max())
        assert (er[ok] <= g.bar_rho[ok]).all(), (key, np.nonzero(ok & (er > g.bar_rho))[0], er[ok].max())


@pytest.mark.parametrize("dew", PROBLEMS)
def test_every_kept_row_is_solved_from_all_three_starts(ctx, dew):
    g = ctx[dew]
    for key, r in g.runs.items():
        missed = np.nonzero(g.c.keep & r["status"])[0]
        assert len(missed) == 0, (key, missed)
        assert (r["iters"][r["status"]] == -1).all() and (r["t"][r["status"]] == 0).all()


@pytest.mark.parametrize("dew", PROBLEMS)
def test_bad_inputs_are_flagged_and_wave_mates_unchanged(ctx, dew):
    from feos_torch_amd import native

    g = ctx[dew]
    c = g.c
    n = 256
    bad = (0.0, -1.0, float("nan"), float("inf"), float("-inf"))
    p, t0 = c.p_spec[:n].copy(), c.T[:n].copy() * 0.93
    rows_p, rows_t = np.arange(3, 3 + 7 * len(bad), 7), np.arange(70, 70 + 11 * len(bad), 11)
    p[rows_p], t0[rows_t] = bad, bad
    a = (_d(c.P[:n]), _d(c.K[:n]))
    r = native.mix_bubble_dew_temperature(*a, _d(p), _d(c.z[:n]), _d(t0), dew, want_iters=True)
    clean = native.mix_bubble_dew_temperature(*a, _d(c.p_spec[:n]), _d(c.z[:n]), _d(c.T[:n] * 0.93), dew, want_iters=True)
    st = r["status"].cpu().numpy()
    assert st[rows_p].all() and st[rows_t].all()
    mates = np.ones(n, dtype=bool)
    mates[rows_p] = mates[rows_t] = False
    m = _d(mates)
    for key in ("t", "rho4", "status", "iters"):
        assert torch.equal(r[key][m], clean[key][m]), key
    assert (r["t"][~m] == 0).all().item() and (r["rho4"][~m] == 0).all().item() and (r["iters"][~m] == -1).all().item()


@pytest.mark.parametrize("dew", PROBLEMS)
def test_solved_rows_are_never_wrong(ctx, dew, oracle):
    g = ctx[dew]
    c = g.c
    for key, r in g.runs.items():
        ok = ~r["status"]
        assert np.isfinite(r["t"][ok]).all() and (r["t"][ok] > 0).all() and np.isfinite(r["rho4"][ok]).all()
        idx = np.nonzero(ok)[0]
        p, _, st = oracle.mix_bubble_dew(c.P[idx], c.K[idx], r["t"][idx], c.z[idx], c.p_spec[idx], dew, prec=1)
        assert not st[c.keep[idx]].any()
        chk = idx[~st]
        err = _rel(p[~st], c.p_spec[chk])
        lim = np.maximum(15.0, np.where(np.isfinite(c.dlnp_dlnT[chk]), c.dlnp_dlnT[chk], 15.0)) * g.bar[chk]
        print("%-7s %-12s start %.2f  oracle p(T) vs p_spec: %.2e on %d rows (%d solved rows the oracle does not answer)" % (
            name(dew), key[0], key[1], err.max(), len(chk), st.sum()))
        assert (err <= lim).all(), (key, chk[err > lim])


@pytest.mark.parametrize("dew", PROBLEMS)
def test_schedule_independence(ctx, dew):
    g = ctx[dew]
    c = g.c
    for s in ref.STARTS:
        a, b = g.runs["as built", s], g.runs["interleaved", s]
        for key in ("t", "rho4", "status", "iters"):
            assert np.array_equal(a[key], b[key]), (s, key)
    full = g.runs["as built", 0.93]
    for n in PREFIXES:
        part = _run(c, dew, np.arange(n), 0.93)
        for key in ("t", "rho4", "status", "iters"):
            assert np.array_equal(part[key], full[key][:n]), (n, key)
    plain = _run(c, dew, np.arange(c.n), 0.93, workspace=False)
    for key in ("t", "rho4", "status", "iters"):
        assert np.array_equal(plain[key], full[key]), key


@pytest.mark.parametrize("dew", PROBLEMS)
def test_start_independence(ctx, dew):
    g = ctx[dew]
    k = g.c.keep
    base = g.runs["as built", 1.0]["t"]
    for s in ref.STARTS[1:]:
        d = _rel(g.runs["as built", s]["t"], base)
        print("%-7s start %.2f vs 1.00: %.2e" % (name(dew), s, d[k].max()))
        assert (d[k] <= 2.0 * g.bar[k]).all()


def _model(c, idx, requires_grad=False):
    from feos_torch_amd import PcSaftMix

    P, K = _d(c.P[idx]).requires_grad_(requires_grad), _d(c.K[idx]).requires_grad_(requires_grad)
    return PcSaftMix(P, K), P, K


@pytest.mark.parametrize("dew", PROBLEMS)
def test_gradients_against_the_referee_quotient(ctx, dew):
    g = ctx[dew]
    c = g.c
    idx = np.arange(c.n)
    eos, P, K = _model(c, idx, True)
    p = _d(c.p_spec).requires_grad_(True)
    z, t0 = _d(c.z).requires_grad_(True), _d(0.93 * c.T).requires_grad_(True)
    T, nans = (eos.dew_temperature if dew else eos.bubble_temperature)(p, z, t0)
    T.sum().backward()
    assert z.grad is None and t0.grad is None
    nans = nans.cpu().numpy()
    got = np.concatenate((P.grad.reshape(c.n, 16).cpu().numpy(), K.grad.cpu().numpy(), p.grad.cpu().numpy()[:, None]), axis=1)
    assert (got[nans] == 0).all(), "dropped rows must receive zero gradient"
    want = ref.quotient(c.grad)
    k = c.keep & ~nans
    err = (np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1))[k]
    print("%-7s gradient: max error %.2e relative to the row's largest component; oracle fp64 vs exact %.2e; dT/dp error %.2e" % (
        name(dew), err.max(), g.e_grad.max(), _rel(got[k, 18], want[k, 18]).max()))
    assert (err <= g.bar_grad[k]).all(), np.nonzero(k)[0][err > g.bar_grad[k]]
    assert (got[~nans, 18] > 0).all(), "dT/dp > 0"
    eos2, P2, _ = _model(c, idx[:8], True)
    T2, _ = (eos2.dew_temperature if dew else eos2.bubble_temperature)(_d(c.p_spec[:8]), _d(c.z[:8]), _d(c.T[:8]))
    (g1,) = torch.autograd.grad(T2.sum(), P2, create_graph=True)
    assert not g1.requires_grad  # once_differentiable: the gradient carries no graph, so a second backward raises
    with pytest.raises(RuntimeError, match="once_differentiable|differentiate twice|does not require grad"):
        g1.sum().backward()


@pytest.mark.parametrize("dew", PROBLEMS)
def test_round_trip_through_the_pressure_solve(ctx, dew):
    g = ctx[dew]
    c = g.c
    idx = np.nonzero(c.keep)[0]
    eos, _, _ = _model(c, idx)
    T, nans = (eos.dew_temperature if dew else eos.bubble_temperature)(_d(c.p_spec[idx]), _d(c.z[idx]), _d(1.07 * c.T[idx]))
    assert not nans.any().item()
    p, nans2 = (eos.dew_point if dew else eos.bubble_point)(T, _d(c.z[idx]), _d(c.p_spec[idx]))
    assert not nans2.any().item()
    err = _rel(p.cpu().numpy(), c.p_spec[idx])
    print("%-7s round trip: %.2e" % (name(dew), err.max()))
    assert (err <= 15.0 * g.bar[idx]).all()


@pytest.mark.parametrize("dew", PROBLEMS)
def test_shell_conventions(ctx, dew):
    from feos_torch_amd import PcSaftMix

    g = ctx[dew]
    c = g.c
    n = 96
    idx = np.arange(n)
    p = c.p_spec[:n].copy()
    p[[5, 50]] = -1.0  # two rows fail
    call = lambda eos, *a, **kw: (eos.dew_temperature if dew else eos.bubble_temperature)(*a, **kw)
    eos, _, _ = _model(c, idx)
    T, nans = call(eos, _d(p), _d(c.z[:n]), _d(c.T[:n]))
    assert T.is_cuda and nans.dtype == torch.bool and nans.shape == (n,) and T.shape == (n - int(nans.sum()),)
    assert nans[5].item() and nans[50].item() and eos._par.shape[0] == T.shape[0] and eos.kij.shape[0] == T.shape[0]
    # CPU tensors in -> CPU tensors out
    cpu = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    eos_c = PcSaftMix(cpu(c.P[:n]), cpu(c.K[:n]))
    Tc, nc = call(eos_c, cpu(p), cpu(c.z[:n]), cpu(c.T[:n]))
    assert not Tc.is_cuda and not nc.is_cuda and torch.equal(Tc, T.cpu()) and torch.equal(nc, nans.cpu())
    # check_stability: same T and nans, stable = stability_analysis of the specified phase at the returned state
    eos_s, _, _ = _model(c, idx)
    Ts, ns, stable = call(eos_s, _d(p), _d(c.z[:n]), _d(c.T[:n]), check_stability=True)
    assert torch.equal(Ts, T) and torch.equal(ns, nans) and stable.dtype == torch.bool and stable.shape == T.shape
    from feos_torch_amd import native

    keep = ~nans
    r = native.mix_bubble_dew_temperature(_d(c.P[:n])[keep], _d(c.K[:n])[keep], _d(p)[keep], _d(c.z[:n])[keep], _d(c.T[:n])[keep], dew)
    assert torch.equal(r["t"], T)
    feed = (r["rho4"][:, 0:2] if dew else r["rho4"][:, 2:4]).contiguous()
    want, _, _ = eos_s.stability_analysis(T, feed)  # eos_s is reduced to the kept rows
    assert torch.equal(stable, want)
    # three components: raises like bubble_point
    eos3 = PcSaftMix(torch.tensor([1.5, 3.5, 250.0, 0, 0, 0, 0, 0], dtype=f64).repeat(2, 3, 1))
    with pytest.raises(Exception, match="binary"):
        call(eos3, cpu(p[:2]), cpu(c.z[:2]), cpu(c.T[:2]))
