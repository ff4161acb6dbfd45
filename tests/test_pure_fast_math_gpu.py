"""GPU: the pure-component kernels on the short fp64 reciprocal and association square root (csrc/dual.hpp, PCS_FAST_RCP == 1
and PCS_FAST_SQRT; the formulas themselves are held to their ulp bounds on the host, tests/test_fast_math_cpu.py).

Rows (tests/tools/fast_math_rows.py): 2,048 = 8 workgroups, 512 of each class alternating row by row, T / T_c over
0.45 ... 0.95, half of the associating rows strongly associating (4 rho Delta >= 40, up to 1e5: the conjugate site-fraction
forms, whose numerator sq - aux cancels).  The oracle alone solves every row (tests/test_fast_math_cpu.py), so every row is
compared and a failed row is a failure of the test: the share of rows left out is 0.  Each comparison runs on the whole
batch and on its first 2,048 - 37 rows (a partial last workgroup).

  * p_sat of pcs_pure_vle_fast + pcs_pure_vle_retry against the long-double oracle at 1e-10 (tests/test_large_parity_gpu.py);
  * rho_V, rho_L of pcs_pure_vle_fp64 and the density of pcs_pure_liquid_density at 2 p_sat at the bars of
    tests/test_saturation_line_gpu.py: max(1e-10, 10 x the oracle's own fp64-vs-long-double discrepancy) at the grid's next
    reduced temperature at or above the row's own (as tests/test_pure_start_eval_gpu.py places rows between grid points);
  * pcs_pure_jacobian, which = 0, 1, 2, against the oracle's exact gradient at the same densities: 1e-12 / 1e-8 / 1e-8 of the
    row's largest component (tests/test_large_parity_gpu.py::test_pure_jacobians_2e5);
  * one launch of the batch and three launches of a third of the rows each give the same bits, for every kernel above.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import fast_math_rows as fr  # noqa: E402
import saturation_grid as sg  # noqa: E402

pytestmark = pytest.mark.gpu

P_BAR = 1e-10
JAC_BARS = {"vapor_pressure": 1e-12, "liquid_density": 1e-8, "equilibrium_liquid_density": 1e-8}  # which = 0, 1, 2
SIZES = (fr.N, fr.PARTIAL)


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(oracle, hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    c = Ctx()
    c.P, c.T, c.theta, c.cls, c.strong = fr.rows(oracle)
    c.p_sat, st_p = oracle.pure_vapor_pressure(c.P, c.T, prec=1)
    c.rho_v, c.rho_l, st_v, _, _ = oracle.pure_vle(c.P, c.T, prec=1)
    c.p_liq = 2.0 * c.p_sat
    c.rho_liq, st_l = oracle.pure_liquid_density(c.P, c.T, c.p_liq, prec=1)
    assert not (st_p | st_v | st_l).any()  # tests/test_fast_math_cpu.py: no row is left out
    grid_theta = np.asarray(sg.SUB)
    theta_up = grid_theta[np.searchsorted(grid_theta, c.theta)]
    cond = sg.reference(orc=oracle)["cond"]  # cached: shared with tests/test_saturation_line_gpu.py in one session
    c.bar = {k: np.array([sg.bar(cond[k], th) for th in theta_up]) for k in ("rho_v", "rho_l", "rho_psat")}
    c.Pd, c.Td, c.pd = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (c.P, c.T, c.p_liq))
    return c


def fast_plus_retry(P, T):
    from feos_torch_amd import native

    plan = native.PureVlePlan(T.shape[0], T.device)
    plan.p_sat.zero_()
    plan.status.fill_(1)
    plan.run_fast(P, T)
    plan.run_retry(P, T)
    torch.cuda.synchronize()
    return {"p_sat": plan.p_sat, "status": plan.status}


def all_fp64(P, T):
    from feos_torch_amd import native

    r = native.pure_vle(P, T, all_fp64=True)
    return {"p_sat": r["p_sat"], "rho_vl": r["rho_vl"], "status": r["status"].view(torch.uint8)}


def liquid(P, T, p):
    from feos_torch_amd import native

    r = native.pure_liquid_density(P, T, p)
    return {"rho": r["rho"], "root": r["rho_root"], "status": r["status"].view(torch.uint8)}


def jacobians(P, T, p):
    """The three Jacobians at the densities of the default solve / the liquid root, with those densities."""
    from feos_torch_amd import native

    r = native.pure_vle(P, T)
    root = native.pure_liquid_density(P, T, p)["rho_root"]
    out = {"rho_vl": r["rho_vl"], "root": root, "status": r["status"].view(torch.uint8)}
    for prop in JAC_BARS:
        if prop == "liquid_density":
            out[prop] = native.pure_jacobian(prop, P, T, p, torch.stack([torch.zeros_like(root), root], dim=1))
        else:
            out[prop] = native.pure_jacobian(prop, P, T, None, r["rho_vl"])
    return out


def _rel(got, want):
    return np.abs(got.cpu().numpy() / want - 1.0)


def _report(name, n, err, bar, c):
    """Prints the figure per class, -> rows over the bar."""
    over = ~(err <= bar)
    for k in range(4):
        m = c.cls[:n] == k
        print("%-28s n %4d %-11s max %.2e (bar %.1e .. %.1e) rows %d" % (name, n, sg.CLASS_NAMES[k], err[m].max(), np.min(bar), np.max(bar), m.sum()))
    if c.strong[:n].any():
        print("%-28s n %4d strong association max %.2e rows %d" % (name, n, err[c.strong[:n]].max(), c.strong[:n].sum()))
    return np.flatnonzero(over)


@pytest.mark.parametrize("n", SIZES)
def test_p_sat_of_fast_plus_retry(ctx, n):
    c = ctx
    r = fast_plus_retry(c.Pd[:n].contiguous(), c.Td[:n].contiguous())
    st = r["status"].cpu().numpy()
    assert not st.any(), np.flatnonzero(st)[:8]  # every row solved: every row is compared
    over = _report("p_sat fast + retry", n, _rel(r["p_sat"], c.p_sat[:n]), P_BAR, c)
    assert len(over) == 0, over[:8]


@pytest.mark.parametrize("n", SIZES)
def test_densities_of_the_all_fp64_kernel(ctx, n):
    c = ctx
    r = all_fp64(c.Pd[:n].contiguous(), c.Td[:n].contiguous())
    assert not r["status"].any().item()
    bad = []
    for j, key in enumerate(("rho_v", "rho_l")):
        over = _report("all-fp64 " + key, n, _rel(r["rho_vl"][:, j], getattr(c, key)[:n]), c.bar[key][:n], c)
        if len(over):
            bad.append((key, over[:8].tolist()))
    over = _report("all-fp64 p_sat", n, _rel(r["p_sat"], c.p_sat[:n]), P_BAR, c)
    assert not bad and len(over) == 0, (bad, over[:8])


@pytest.mark.parametrize("n", SIZES)
def test_liquid_density_at_twice_p_sat(ctx, n):
    c = ctx
    r = liquid(c.Pd[:n].contiguous(), c.Td[:n].contiguous(), c.pd[:n].contiguous())
    assert not r["status"].any().item()
    over = _report("liquid density at 2 p_sat", n, _rel(r["rho"], c.rho_liq[:n]), c.bar["rho_psat"][:n], c)
    assert len(over) == 0, over[:8]


@pytest.mark.parametrize("n", SIZES)
def test_jacobians_against_the_exact_gradient_at_the_same_densities(ctx, oracle, n):
    c = ctx
    r = jacobians(c.Pd[:n].contiguous(), c.Td[:n].contiguous(), c.pd[:n].contiguous())
    assert not r["status"].any().item()
    rho_vl, root = r["rho_vl"].cpu().numpy(), r["root"].cpu().numpy()
    P, T = np.ascontiguousarray(c.P[:n]), np.ascontiguousarray(c.T[:n])
    bad = []
    for prop, bar in JAC_BARS.items():
        if prop == "liquid_density":
            _, want = oracle.pure_property_grad(prop, P, T, np.ascontiguousarray(c.p_liq[:n]), None, root, exact=True)
        else:
            _, want = oracle.pure_property_grad(prop, P, T, None, rho_vl[:, 0].copy(), rho_vl[:, 1].copy(), exact=True)
        J = r[prop].cpu().numpy()
        assert np.isfinite(J).all()
        err = (np.abs(J - want) / np.abs(want).max(axis=1, keepdims=True)).max(axis=1)
        over = _report("jacobian " + prop, n, err, bar, c)
        if len(over):
            bad.append((prop, over[:8].tolist()))
    assert not bad, bad


def test_one_launch_and_three_launches_of_a_third_give_the_same_bits(ctx):
    c = ctx
    cuts = (0, 683, 1366, fr.N)
    runs = {"fast + retry": lambda a, b: fast_plus_retry(c.Pd[a:b].contiguous(), c.Td[a:b].contiguous()),
            "all-fp64": lambda a, b: all_fp64(c.Pd[a:b].contiguous(), c.Td[a:b].contiguous()),
            "liquid density": lambda a, b: liquid(c.Pd[a:b].contiguous(), c.Td[a:b].contiguous(), c.pd[a:b].contiguous()),
            "jacobians": lambda a, b: jacobians(c.Pd[a:b].contiguous(), c.Td[a:b].contiguous(), c.pd[a:b].contiguous())}
    bad = []
    for name, run in runs.items():
        whole = run(0, fr.N)
        parts = [run(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
        for key, w in whole.items():
            joined = torch.cat([p[key] for p in parts], dim=0)
            same = torch.equal(w.contiguous().view(torch.uint8), joined.contiguous().view(torch.uint8))
            print("%-14s %-26s one launch == three launches: %s" % (name, key, same))
            if not same:
                bad.append((name, key, int((w != joined).sum().item())))
    assert not bad, bad
