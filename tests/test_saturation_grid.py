"""CPU: what the reference alone does on the saturation-line grid (tests/tools/saturation_grid.py), so that every assertion
of tests/test_saturation_line_gpu.py is one the oracle itself satisfies.

800 rows of all four classes at theta = T / T_c from 0.45 to 0.9999 (sub-critical) and 1.0001 to 1.03 (super-critical),
T_c, p_c, rho_c from the oracle scan of tests/tools/critical_referee.py.  Measured (long double / fp64 identical):
every sub-critical row solved and every super-critical row failed by pure_vle, pure_vapor_pressure and
pure_equilibrium_liquid_density; p_sat fp64 vs long double <= 1.3e-13 everywhere (1.1e-13 at 0.9999);
rho_V / rho_L fp64 vs long double 1.3e-13 / 7e-14 at 0.45, 1.7e-12 / 1.1e-12 at 0.999, 4.5e-11 / 3.9e-11 at 0.9999.

The two liquid_density cases, p = 1.05 p_sat(theta) and p = 2 p_c: the oracle solves every sub-critical row of both (and,
with p = 1.05 p_c in place of the first, every super-critical row too: a dense root exists at any temperature), so both
cases stay in the grid as the issue states them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import saturation_grid as sg  # noqa: E402


@pytest.fixture(scope="module")
def data(oracle):
    g = sg.grid(orc=oracle)
    return g, sg.reference(orc=oracle)


def test_grid_shape_and_orders(data):
    g, _ = data
    n = sg.N_ROWS * len(sg.THETA)
    assert g.P.shape == (n, 8) and all(len(x) == n for x in g[1:])
    assert len(sg.SUB) == 11 and len(sg.SUPER) == 4 and n == 12_000
    cls = sg.classes(g.P[: sg.N_ROWS])
    assert all((cls == c).sum() >= 150 for c in range(4)), np.bincount(cls)
    for th, sl in sg.theta_slices(g):  # theta-major: whole waves at one theta
        assert (g.theta[sl] == th).all() and np.array_equal(g.row[sl], np.arange(sg.N_ROWS))
        assert np.array_equal(g.T[sl], th * g.Tc[sl])
    perm = sg.interleave(n)
    assert np.array_equal(np.sort(perm), np.arange(n)) and np.array_equal(perm, sg.interleave(n))
    th, cl = g.theta[perm], sg.classes(g.P[perm])
    for w in range(n // 64):  # interleaved: every wave mixes sub- and super-critical rows and at least three classes
        s = slice(64 * w, 64 * w + 64)
        assert th[s].min() < 0.99 and th[s].max() > 1.0 and len(set(cl[s])) >= 3, w


@pytest.mark.parametrize("prec", ["ld", "f64"])
def test_oracle_solves_the_sub_critical_grid_and_nothing_above(data, prec):
    g, ref = data
    r, sub = ref[prec], sg.sub_mask(g)
    for key in ("st_vle", "st_p", "st_eq"):
        assert not r[key][sub].any(), (key, g.theta[sub][r[key][sub]])
        assert r[key][~sub].all(), (key, g.theta[~sub][~r[key][~sub]])
    assert (r["p_sat"][sub] > 0).all() and (r["p_sat"][sub] < g.pc[sub]).all()
    assert (r["rho_v"][sub] > 0).all()
    assert (r["rho_v"][sub] < g.rhoc_red[sub]).all() and (g.rhoc_red[sub] < r["rho_l"][sub]).all()
    assert (r["rho_eq"][sub] > g.rhoc[sub]).all()


@pytest.mark.parametrize("case", ["psat", "pc"])
@pytest.mark.parametrize("prec", ["ld", "f64"])
def test_oracle_liquid_density_cases(data, prec, case):
    g, ref = data
    r, sub = ref[prec], sg.sub_mask(g)
    assert not r["st_" + case][sub].any()
    assert (r["rho_" + case][sub] > g.rhoc[sub]).all()
    assert (r["root_" + case][sub] > g.rhoc_red[sub]).all()
    if case == "psat":  # compressed liquid: denser than the saturated one
        assert (r["rho_psat"][sub] > ref["ld"]["rho_eq"][sub]).all()


def test_conditioning_table(data):
    """The table of the issue: p_sat is well conditioned up to 0.9999 (no allowance on the 1e-10 bar), the densities are not."""
    g, ref = data
    c = ref["cond"]
    for th in sg.SUB:
        print("theta %-7g gap %.3f  fp64 vs long double: p_sat %.1e rho_V %.1e rho_L %.1e rho_eq %.1e rho(1.05 p_sat) %.1e "
              "rho(2 p_c) %.1e | exact gradient at the fp64 vs long-double root: p_sat %.1e rho_eq %.1e"
              % (th, c["gap"][th], c["p_sat"][th], c["rho_v"][th], c["rho_l"][th], c["rho_eq"][th], c["rho_psat"][th],
                 c["rho_pc"][th], c["grad_vapor_pressure"][th], c["grad_equilibrium_liquid_density"][th]))
        assert c["p_sat"][th] < 1e-12
        for key in ("rho_v", "rho_l", "rho_eq", "rho_psat", "rho_pc"):
            assert sg.bar(c[key], th) < 1e-8  # the bars stay meaningful: at most 100 x the project's 1e-10
    assert c["gap"][0.45] > 0.99 and 0.02 < c["gap"][0.9999] < 0.04
    assert all(np.isnan(c["rho_v"][th]) for th in sg.SUPER)
