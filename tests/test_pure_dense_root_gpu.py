"""GPU: the dense-side entry of the fp32 liquid root (csrc/pure_f32.hpp: liquid_root_step, liquid_root_f32).

A lane whose zero-pressure liquid lies above the start packing fraction eta = 0.5 restarts on the dense side of its root: at
the plain Newton point from eta = 0.5 where that point is usable, else on the ladder eta = 0.58, 0.66, 0.74.  The batch is built
so that this code runs: 600 rows (two full 256-row workgroups and a partial one), every second one a strongly polar row at
low temperature (half of them associating, drawn as the association-flag corner rows of tests/test_pure_lean_presolve_gpu.py
with mu in [2.6, 3] D and T/T_c in [0.55, 0.62]) whose zero-pressure liquid the oracle puts above eta = 0.5, at least 20 of
them above eta = 0.58 (the rows that needed a second rung of the ladder); the others are ordinary rows of the benchmark's
distribution, so the waves hold both kinds.

  * status and p_sat of pcs_pure_vle (pressure-only kernel) against the long-double oracle: 1e-10 relative, the bar of
    tests/test_saturation_line_gpu.py, for dense-side and ordinary rows alike; the oracle solves every row (checked when the
    rows are chosen), none is skipped;
  * pcs_pure_liquid_density at p = 2 p_sat (the same liquid root with p_spec != 0) against the oracle at the 1e-9 of
    tests/test_pure_gpu.py;
  * one launch of 600 rows against three launches of 200: p_sat bit-identical (a row's result does not depend on its
    wave-mates);
  * the main kernel hands none of the rows to the all-fp64 fallback or to the robust pass.

Mutation check (variant builds, MI355X): with the guard eta(rho_1) <= 0.74 removed 2 of the 4 tests fail (liquid density of a
row with eta = 0.605 off by a factor of 3.5, 41 rows in the fallback list); taking the entry also when dp/drho <= 0 changes
nothing, the interval guard already rejects those Newton points.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

P_BAR = 1e-10  # p_sat against the long-double oracle (tests/test_saturation_line_gpu.py::P_BAR)
RHO_BAR = 1e-9  # liquid_density against the oracle (tests/test_pure_gpu.py::RTOL)
N_ROWS, N_DENSE, N_SECOND_RUNG = 600, 300, 20
POOL = 40_000


def packing_fraction_factor(P, T):
    d = P[:, 1] * (1.0 - 0.12 * np.exp(-3.0 * P[:, 2] / T))
    return np.pi / 6.0 * P[:, 0] * d ** 3


def zero_pressure_liquid_eta(orc, P, T):
    """Packing fraction of the zero-pressure liquid: plain Newton on the oracle's (p, dp/drho) from eta = 0.74, monotone
    from above on the convex liquid branch.  -> eta, converged mask."""
    ceta = packing_fraction_factor(P, T)
    rho = 0.74 / ceta
    ok = np.ones(len(T), dtype=bool)
    conv = np.zeros(len(T), dtype=bool)
    with np.errstate(all="ignore"):
        for _ in range(60):
            _, p, dp = orc.pure_derivatives(P, T, rho)
            step = p / dp
            ok &= np.isfinite(step) & (dp > 0.0) & (rho - step > 0.0)
            conv = np.abs(step) <= 1e-12 * rho
            rho = np.where(ok, rho - step, rho)
            if conv[ok].all():
                break
    return rho * ceta, ok & conv


def dense_candidates(orc):
    """Strongly polar low-temperature corner rows whose liquid at eta = 0.5 is under tension (p < 0, dp/drho > 0)."""
    from test_pure_lean_presolve_gpu import corner_rows

    P, _ = corner_rows(POOL, seed=6061)
    rng = np.random.default_rng(11)
    P[:, 3] = rng.uniform(2.6, 3.0, POOL)
    T = P[:, 2] * 1.28 * P[:, 0] ** 0.45 * rng.uniform(0.55, 0.62, POOL)
    _, p, dp = orc.pure_derivatives(P, T, 0.5 / packing_fraction_factor(P, T))
    cand = (p < 0.0) & (dp > 0.0)
    return np.ascontiguousarray(P[cand]), np.ascontiguousarray(T[cand])


def solved_by_the_oracle(orc, P, T):
    """-> p_sat, liquid density at 2 p_sat, mask of the rows the long-double oracle solves for both."""
    p_sat, st = orc.pure_vapor_pressure(P, T, prec=1)
    pp = np.where(st, 1e5, 2.0 * p_sat)
    rho, st_rho = orc.pure_liquid_density(P, T, pp, prec=1)
    return p_sat, rho, ~st & ~st_rho & np.isfinite(p_sat) & (p_sat > 0.0)


class Ctx:
    pass


def build_rows(orc):
    """The 600 rows with their oracle values: dense-side rows at the even positions, ordinary rows at the odd ones."""
    from feos_torch_amd.synthetic import pure_batch

    Pd_, Td_ = dense_candidates(orc)
    eta, conv = zero_pressure_liquid_eta(orc, Pd_, Td_)
    p_d, rho_d, ok_d = solved_by_the_oracle(orc, Pd_, Td_)
    keep = np.flatnonzero(conv & ok_d & (eta > 0.5))
    second = keep[eta[keep] > 0.58]
    first = keep[eta[keep] <= 0.58]
    n_second = min(len(second), N_DENSE // 3)
    rows = np.concatenate([second[:n_second], first[:N_DENSE - n_second]])
    rows = rows[np.random.default_rng(5).permutation(len(rows))]  # the second-rung rows spread over the workgroups
    # the generator's own guarantee: the batch enters the dense-side code, and the part of it behind the first rung
    assert len(rows) == N_DENSE and (eta[rows] > 0.5).sum() >= 100 and (eta[rows] > 0.58).sum() >= N_SECOND_RUNG, (len(rows), n_second)
    Po, To = pure_batch(N_ROWS - N_DENSE + 100, seed=6062)
    p_o, rho_o, ok_o = solved_by_the_oracle(orc, Po, To)
    ordinary = np.flatnonzero(ok_o)[:N_ROWS - N_DENSE]
    assert len(ordinary) == N_ROWS - N_DENSE
    c = Ctx()
    c.P, c.T, c.p_sat, c.rho = np.empty((N_ROWS, 8)), np.empty(N_ROWS), np.empty(N_ROWS), np.empty(N_ROWS)
    c.eta = np.zeros(N_ROWS)  # 0: ordinary row
    for dst, src, idx in ((slice(0, None, 2), (Pd_, Td_, p_d, rho_d), rows), (slice(1, None, 2), (Po, To, p_o, rho_o), ordinary)):
        c.P[dst], c.T[dst], c.p_sat[dst], c.rho[dst] = (a[idx] for a in src)
    c.eta[0::2] = eta[rows]
    print("dense-side rows %d (eta > 0.58: %d, max eta %.3f), ordinary rows %d" % ((c.eta > 0.5).sum(), (c.eta > 0.58).sum(), c.eta.max(), (c.eta == 0).sum()))
    return c


@pytest.fixture(scope="module")
def ctx(oracle, hip_lib):
    from feos_torch_amd import native

    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    c = build_rows(oracle)
    c.Pd, c.Td = torch.from_numpy(c.P).cuda(), torch.from_numpy(c.T).cuda()
    c.native = native
    c.res = native.pure_vle(c.Pd, c.Td, want_rho_vl=False)
    return c


def test_p_sat_and_status_against_the_long_double_oracle(ctx):
    c = ctx
    st = c.res["status"].cpu().numpy()
    assert not st.any(), ("rows the oracle solves are reported failed", np.flatnonzero(st)[:8].tolist(), c.eta[st][:8].tolist())
    err = np.abs(c.res["p_sat"].cpu().numpy() / c.p_sat - 1.0)
    for name, rows in (("ordinary", c.eta == 0.0), ("eta in (0.5, 0.58]", (c.eta > 0.5) & (c.eta <= 0.58)), ("eta > 0.58", c.eta > 0.58)):
        print("p_sat %-20s rows %3d bar %.1e measured %.2e" % (name, rows.sum(), P_BAR, err[rows].max()))
    assert err.max() <= P_BAR, (float(err.max()), int(err.argmax()), float(c.eta[err.argmax()]))


def test_liquid_density_at_twice_p_sat_against_the_oracle(ctx):
    c = ctx
    r = c.native.pure_liquid_density(c.Pd, c.Td, torch.from_numpy(2.0 * c.p_sat).cuda())
    st = r["status"].cpu().numpy()
    assert not st.any(), (np.flatnonzero(st)[:8].tolist(), c.eta[st][:8].tolist())
    err = np.abs(r["rho"].cpu().numpy() / c.rho - 1.0)
    for name, rows in (("ordinary", c.eta == 0.0), ("eta > 0.5", c.eta > 0.5)):
        print("liquid density %-10s rows %3d bar %.1e measured %.2e" % (name, rows.sum(), RHO_BAR, err[rows].max()))
    assert err.max() <= RHO_BAR, (float(err.max()), int(err.argmax()), float(c.eta[err.argmax()]))


def test_one_launch_and_three_launches_give_the_same_bits(ctx):
    c = ctx
    whole = c.res["p_sat"].cpu().numpy()
    for k in range(3):
        part = c.native.pure_vle(c.Pd[200 * k:200 * (k + 1)].contiguous(), c.Td[200 * k:200 * (k + 1)].contiguous(), want_rho_vl=False)
        assert not part["status"].any().item()
        assert np.array_equal(part["p_sat"].cpu().numpy().view(np.uint64), whole[200 * k:200 * (k + 1)].view(np.uint64)), k


def test_no_row_leaves_the_main_kernel(ctx):
    """The rows are the main kernel's own: the oracle solves them and their temperatures lie inside the benchmark's range,
    where the main kernel hands no row of 1e7 to the all-fp64 fallback or the robust pass.  A dense-side start that misbehaves
    (a Newton point beyond close packing, say) sends its lane to the fallback, where it still gets the right p_sat: only
    this count shows it."""
    c = ctx
    plan = c.native.PureVlePlan(N_ROWS, c.Td.device)
    plan.run_fast(c.Pd, c.Td)
    torch.cuda.synchronize()
    fallback, robust = plan.retry_count()
    print("main-kernel lists: fallback %d robust %d" % (fallback, robust))
    assert fallback == 0 and robust == 0
