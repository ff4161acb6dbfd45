"""GPU: PcSaftPure.critical_point / pcs_pure_critical_point(_vjp) against the two CPU referees of
tests/tools/critical_referee.py (mpmath: exact on every class; oracle scan: independent of the kernels' formulation), against
the oracle's own dp/drho, against the existing VLE kernels, and their gradients, edge rows and hipGraph capture.

Bars: T_c, p_c and rho_c (against mpmath) at the project's 1e-10 for properties; rho_c against the scan at
the scan's own resolution (critical_referee.SCAN_RHO_RESOLUTION); gradients at 1e-7 of the row's largest component against
the exact mpmath gradient and 1e-4 against central differences of the scan."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import critical_referee as cr  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL = 1e-10
f64 = torch.float64


@pytest.fixture(scope="module")
def amd():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import feos_torch_amd

    return feos_torch_amd


def _solve(P, t_init=None, want_iters=False):
    from feos_torch_amd import native

    dev = torch.device("cuda:0")
    r = native.pure_critical_point(torch.from_numpy(P).to(dev), None if t_init is None else torch.from_numpy(t_init).to(dev),
                                   want_iters=want_iters)
    return {k: (None if v is None else v.cpu().numpy()) for k, v in r.items()}


def _rel(a, b):
    return np.abs(a / b - 1.0)


def test_parity_with_the_oracle_scan_all_classes(amd, oracle):
    P = cr.sample(2400, seed=cr.SCAN_SEED)
    polar, assoc = P[:, 3] != 0, P[:, 4] != 0
    for a in (False, True):
        for b in (False, True):
            assert ((polar == a) & (assoc == b)).sum() >= 300
    Tc, pc, rc, _ = cr.oracle_scan(oracle, P)
    r = _solve(P)
    print("vs scan, max rel: T_c %.3e p_c %.3e rho_c %.3e" % (_rel(r["t_c"], Tc).max(), _rel(r["p_c"], pc).max(), _rel(r["rho_c"], rc).max()))
    assert not r["status"].any(), np.where(r["status"])[0]
    assert _rel(r["t_c"], Tc).max() <= RTOL
    assert _rel(r["p_c"], pc).max() <= RTOL
    assert _rel(r["rho_c"], rc).max() <= cr.SCAN_RHO_RESOLUTION
    # the same through the model class: nothing dropped, same numbers
    par = torch.from_numpy(P).to("cuda:0")
    eos = amd.PcSaftPure(par)
    nans, t_c, p_c, rho_c = eos.critical_point()
    assert nans.dtype == torch.bool and not nans.any().item() and t_c.device == par.device
    assert np.array_equal(t_c.cpu().numpy(), r["t_c"]) and np.array_equal(p_c.cpu().numpy(), r["p_c"])
    assert np.array_equal(rho_c.cpu().numpy(), r["rho_c"])


def test_parity_with_mpmath(amd, oracle):
    """240 mu = 0 rows (non-polar and associating) and 60 polar rows against the 50-digit referee."""
    P = np.concatenate([cr.sample(240, seed=cr.MP_SEED, mu_zero=True), cr.sample(60, seed=cr.MP_SEED, mu_zero=False)])
    r = _solve(P)
    assert not r["status"].any()
    e = np.zeros((len(P), 3))
    for i in range(len(P)):
        T, p, rho, p3 = cr.mp_critical(P[i], r["t_c"][i], r["rho_c"][i] * cr.RHO_UNIT)
        assert p3 > 0
        e[i] = [abs(r["t_c"][i] / float(T) - 1), abs(r["p_c"][i] / float(p) - 1), abs(r["rho_c"][i] * cr.RHO_UNIT / float(rho) - 1)]
    print("vs mpmath, max rel: T_c %.3e p_c %.3e rho_c %.3e" % tuple(e.max(axis=0)))
    assert e.max() <= RTOL, e.max(axis=0)


def test_residuals_against_the_oracle_alone(amd, oracle):
    """No referee: the oracle's dp/drho at the returned point is zero to the rounding of its own evaluation, and positive
    on either side."""
    P = cr.sample(2400, seed=cr.SCAN_SEED)
    r = _solve(P)
    T, rho = r["t_c"], r["rho_c"] * cr.RHO_UNIT
    dp = oracle.pure_derivatives(P, T, rho)[2]
    noise = cr.dp_noise(oracle, P, T, rho)
    print("max |dp/drho| %.3e, max |dp/drho| / bound %.3f" % (np.abs(dp).max(), (np.abs(dp) / noise).max()))
    assert (np.abs(dp) <= noise).all()
    for s in (1.0 - 1e-3, 1.0 + 1e-3):
        assert (oracle.pure_derivatives(P, T, rho * s)[2] > 0).all(), s


def test_consistency_with_the_vle_kernels(amd):
    P = cr.vle_sample()
    par = torch.from_numpy(P).to("cuda:0")
    nans, t_c, p_c, rho_c = amd.PcSaftPure(par).critical_point()
    assert not nans.any().item()
    nans, p_sat = amd.PcSaftPure(par).vapor_pressure(cr.F_SUB * t_c)
    assert not nans.any().item() and (p_sat < p_c).all().item() and (p_sat > 0).all().item()
    nans, rho_l = amd.PcSaftPure(par).equilibrium_liquid_density(cr.F_SUB * t_c)
    assert not nans.any().item() and (rho_l > rho_c).all().item()
    nans, _ = amd.PcSaftPure(par).vapor_pressure(1.03 * t_c)
    assert nans.all().item()


def _grads_abi(P, tc, rc):
    from feos_torch_amd import native

    dev = torch.device("cuda:0")
    n = len(P)
    one, out = torch.ones(n, dtype=f64, device=dev), []
    for o in range(3):
        g = [None, None, None]
        g[o] = one
        out.append(native.pure_critical_point_vjp(torch.from_numpy(P).to(dev), torch.from_numpy(tc).to(dev),
                                                  torch.from_numpy(rc).to(dev), *g).cpu().numpy())
    return np.stack(out, axis=1)  # [n, 3, 8]


def test_gradients_against_mpmath(amd):
    P = np.concatenate([cr.sample(24, seed=cr.MP_SEED + 1, mu_zero=True), cr.sample(8, seed=cr.MP_SEED + 1, mu_zero=False)])
    r = _solve(P)
    assert not r["status"].any()
    G = _grads_abi(P, r["t_c"], r["rho_c"])
    worst = 0.0
    for i in range(len(P)):
        T, p, rho, _ = cr.mp_critical(P[i], r["t_c"][i], r["rho_c"][i] * cr.RHO_UNIT)
        E = cr.mp_gradient(P[i], T, rho)
        for o in range(3):
            worst = max(worst, np.abs(G[i, o] - E[o]).max() / np.abs(E[o]).max())
    print("gradient vs mpmath, max error / largest component %.3e" % worst)
    assert worst <= 1e-7


def test_gradients_against_scan_differences_on_polar_rows(amd, oracle):
    P = cr.sample(48, seed=cr.SCAN_SEED + 1, mu_zero=False)
    r = _solve(P)
    assert not r["status"].any()
    G = _grads_abi(P, r["t_c"], r["rho_c"])
    FD = cr.scan_central_differences(oracle, P)
    # T_c and p_c: the scan is sharp (1e-14), a central difference with a relative step of 1e-4 carries ~1e-8 of truncation.
    # rho_c: the scan resolves 6e-8, i.e. 6e-4 of a 1e-4 step: no finite-difference check at 1e-4 is possible there, the
    # exact mpmath gradient above covers it on polar rows too.
    worst = 0.0
    for o in range(2):
        scale = np.abs(FD[:, o]).max(axis=1)
        worst = max(worst, (np.abs(G[:, o] - FD[:, o]).max(axis=1) / scale).max())
    print("gradient vs scan differences, max error / largest component %.3e" % worst)
    assert worst <= 1e-4


def test_autograd_equals_the_abi_and_failed_rows_get_zero(amd):
    P = cr.sample(64, seed=21)
    P[5] = np.nan
    P[17, 0] = -1.0
    P[40, 0] = 0.0
    bad = np.zeros(64, dtype=bool)
    bad[[5, 17, 40]] = True
    par = torch.from_numpy(P).to("cuda:0").requires_grad_(True)
    eos = amd.PcSaftPure(par)
    nans, t_c, p_c, rho_c = eos.critical_point()
    assert np.array_equal(nans.cpu().numpy(), bad)
    assert t_c.shape == p_c.shape == rho_c.shape == (61,) and eos.parameters.shape == (61, 8)
    w = torch.linspace(0.5, 1.5, 61, dtype=f64, device="cuda:0")
    (w * t_c).sum().backward(retain_graph=True)
    g_t = par.grad.clone()
    par.grad = None
    (w * t_c * 1e-2 + p_c * 1e-6 * w - 3.0 * rho_c).sum().backward()
    g_all = par.grad.cpu().numpy()
    assert (g_all[bad] == 0).all() and (g_t.cpu().numpy()[bad] == 0).all() and np.isfinite(g_all).all()
    # the C ABI with the cotangents autograd hands to the backward pass: the same kernel on the same inputs
    from feos_torch_amd import native

    good = torch.from_numpy(P[~bad]).to("cuda:0")
    tc_d, rc_d = t_c.detach(), rho_c.detach()
    abi_t = native.pure_critical_point_vjp(good, tc_d, rc_d, g_tc=w).cpu().numpy()
    abi_all = native.pure_critical_point_vjp(good, tc_d, rc_d, g_tc=w * 1e-2, g_pc=1e-6 * w,
                                             g_rhoc=torch.full_like(w, -3.0)).cpu().numpy()
    for got, want in ((g_t.cpu().numpy()[~bad], abi_t), (g_all[~bad], abi_all)):
        err = np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)
        print("autograd vs C ABI, max error / largest component %.3e" % err.max())
        assert err.max() <= 1e-14
    # and the product rule: w_T dT_c + w_p dp_c + w_rho drho_c from the three unit-cotangent calls (each entry a sum of
    # three products with cancellation: compared at 1e-12 of the row's largest term)
    G = _grads_abi(P[~bad], tc_d.cpu().numpy(), rc_d.cpu().numpy())
    wn = w.cpu().numpy()[:, None]
    terms = np.stack([1e-2 * wn * G[:, 0], 1e-6 * wn * G[:, 1], -3.0 * G[:, 2]])
    scale = np.abs(terms).max(axis=(0, 2))
    assert (np.abs(g_all[~bad] - terms.sum(axis=0)).max(axis=1) <= 1e-12 * scale).all()
    assert (np.abs(g_t.cpu().numpy()[~bad] - wn * G[:, 0]).max(axis=1) <= 1e-12 * np.abs(wn * G[:, 0]).max(axis=1)).all()


def test_edge_rows_shapes_and_initial_temperature(amd):
    from feos_torch_amd import native

    P = cr.sample(700, seed=23)
    edge = {3: (0, np.nan), 64: (2, np.inf), 65: (0, -2.0), 300: (0, 0.0), 301: (1, -3.5), 699: (2, 0.0)}
    for row, (col, val) in edge.items():
        P[row, col] = val
    bad = np.zeros(700, dtype=bool)
    bad[list(edge)] = True
    r = _solve(P, want_iters=True)  # returns: every loop is capped
    assert np.array_equal(r["status"], bad)
    assert (r["t_c"][bad] == 0).all() and (r["iters"][bad] == -1).all() and (r["iters"][~bad] <= 30).all()
    eos = amd.PcSaftPure(torch.from_numpy(P))  # CPU tensors are accepted, results come back on the CPU
    nans, t_c, p_c, rho_c = eos.critical_point()
    assert nans.shape == (700,) and nans.dtype == torch.bool and not nans.is_cuda and not t_c.is_cuda
    assert np.array_equal(nans.numpy(), bad) and t_c.shape == p_c.shape == rho_c.shape == (694,)
    assert eos.parameters.shape == (694, 8) and np.array_equal(eos.parameters, P[~bad])
    assert np.array_equal(t_c.numpy(), r["t_c"][~bad])
    G = P[~bad]
    # partial workgroups (idle lanes repeat the last row): 1 and 257 rows alone equal the same rows of a 512-row call bit
    # for bit, solve and gradient
    dev = torch.device("cuda:0")
    full = _solve(G[:512])
    tc, rc = torch.from_numpy(full["t_c"]).to(dev), torch.from_numpy(full["rho_c"]).to(dev)
    w = torch.linspace(0.5, 1.5, 512, dtype=f64, device=dev)
    grad = lambda m: native.pure_critical_point_vjp(torch.from_numpy(G[:m]).to(dev), tc[:m], rc[:m], g_tc=w[:m], g_pc=1e-6 * w[:m],
                                                     g_rhoc=-3.0 * w[:m])
    g_full = grad(512)
    assert not full["status"].any() and torch.isfinite(g_full).all().item()
    for m in (1, 257):
        part = _solve(G[:m])
        for k in ("t_c", "p_c", "rho_c"):
            assert np.array_equal(part[k].view(np.int64), full[k][:m].view(np.int64)), (m, k)
        assert not part["status"].any()
        assert torch.equal(grad(m).view(torch.int64), g_full[:m].view(torch.int64)), m
    # a supplied start within +-30 % of T_c: same point
    t0 = r["t_c"][~bad] * np.random.default_rng(5).uniform(0.7, 1.3, len(G))
    nans2, t2, p2, rho2 = amd.PcSaftPure(torch.from_numpy(G)).critical_point(initial_temperature=torch.from_numpy(t0))
    assert not nans2.any().item()
    for a, b in ((t2, t_c), (p2, p_c), (rho2, rho_c)):
        assert _rel(a.numpy(), b.numpy()).max() <= 1e-12
    with pytest.raises(ValueError, match="initial_temperature has 3 rows"):
        native.pure_critical_point(torch.from_numpy(G).to("cuda:0"), torch.ones(3, dtype=f64, device="cuda:0"))


def test_hipgraph_replay_behind_pending_work_equals_eager(amd):
    """Forward + vjp are plain kernel sequences: a capture replayed behind pending launches reproduces the eager bits."""
    from feos_torch_amd import native
    from feos_torch_amd.synthetic import pure_batch

    n = 200_000
    P, _ = pure_batch(n, seed=613)
    P[7] = np.nan
    dev = torch.device("cuda:0")
    par = torch.from_numpy(P).to(dev)
    g = [torch.full((n,), v, dtype=f64, device=dev) for v in (1.0, 1e-6, -2.0)]

    def run():
        r = native.pure_critical_point(par)
        return r, native.pure_critical_point_vjp(par, r["t_c"], r["rho_c"], *g)

    r0, gp0 = run()
    torch.cuda.synchronize()
    ref = [t.clone() for t in (r0["t_c"], r0["p_c"], r0["rho_c"], r0["status"].view(torch.uint8), gp0)]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        r1, gp1 = run()
    outs = (r1["t_c"], r1["p_c"], r1["rho_c"], r1["status"].view(torch.uint8), gp1)
    for rep in range(3):
        for t in outs:
            t.fill_(7) if t.dtype == torch.uint8 else t.fill_(float("nan"))
        for _ in range(3):  # pending work ahead of the replay
            native.pure_critical_point(par)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, ref):
            assert torch.equal(got, want) or (got.dtype == f64 and torch.equal(got.view(torch.int64), want.view(torch.int64))), rep
