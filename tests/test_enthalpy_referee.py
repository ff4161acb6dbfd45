"""CPU: the two referees of the enthalpy of vaporization (tests/tools/enthalpy_referee.py) agree with each other, so the GPU
tests can lean on either.  24 rows: 2 parameter rows of each of the four classes at theta = T / T_c in {0.6, 0.9, 0.99}.

(a) the Clausius-Clapeyron value from the long-double oracle (its densities, its dp_sat/dT) against (b) the direct form at the
    50-digit mpmath equilibrium: <= 1e-12.  Measured here: 4.2e-15 (theta = 0.99; 4.4e-16 at 0.6 and 0.9), so the oracle's
    double-rounded densities ask for no more than the issue's bound.
(c) the mpmath gradient (implicit-function theorem) against central differences of the whole mpmath solve, relative to the
    row's largest component: both are exact to ~1e-18 (steps and precision in the referee), asserted at 1e-15; and the
    fast evaluation the gradient differentiates against the mp.diff forms of the value and the equilibrium conditions.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import critical_referee as cr  # noqa: E402
import enthalpy_referee as er  # noqa: E402


@pytest.fixture(scope="module")
def rows(oracle):
    P0 = er.referee_rows(2)
    assert sorted(set((P0[:, 3] != 0) + 2 * (P0[:, 4] != 0))) == [0, 1, 2, 3]
    Tc, _, _, _ = cr.oracle_scan(oracle, P0)
    P = np.ascontiguousarray(np.tile(P0, (len(er.REFEREE_THETA), 1)))
    T = np.concatenate([th * Tc for th in er.REFEREE_THETA])
    dh, rv, rl, st = er.cc_value(oracle, P, T)
    assert len(T) == 24 and not st.any()
    return P, T, dh, rv, rl


def test_clausius_clapeyron_oracle_equals_the_direct_form_in_mpmath(rows):
    P, T, dh, rv, rl = rows
    exact = np.array([float(er.mp_value(P[i], T[i], rv[i], rl[i])) for i in range(len(T))])
    err = np.abs(dh - exact) / exact
    for k, th in enumerate(er.REFEREE_THETA):
        print("theta %-5g (a) vs (b): max rel %.2e" % (th, err[8 * k:8 * k + 8].max()))
    print("largest relative difference %.3e" % err.max())
    assert (exact > 0).all() and err.max() <= 1e-12
    # the mpmath equilibrium is the oracle's to the oracle's own rounding
    for i in (0, 9, 23):
        v, l = er.mp_equilibrium(P[i], T[i], rv[i], rl[i])
        assert abs(rv[i] / float(v) - 1) <= 1e-11 and abs(rl[i] / float(l) - 1) <= 1e-11


def test_mpmath_gradient_equals_central_differences_of_the_whole_solve(rows):
    P, T, dh, rv, rl = rows
    worst = 0.0
    for i in range(len(T)):
        g = er.mp_gradient(P[i], T[i], rv[i], rl[i])
        c = er.mp_central_difference(P[i], T[i], rv[i], rl[i])
        assert np.isfinite(g).all()
        worst = max(worst, np.abs(g - c).max() / np.abs(g).max())
    print("gradient vs central differences of the solve, max error / largest component %.3e" % worst)
    assert worst <= 1e-15


def test_fast_evaluation_equals_the_mp_diff_forms(rows):
    P, T, dh, rv, rl = rows
    mp = cr._mp()
    for i in (1, 12, 22):
        par, t = er._mpf_row(mp, P[i], T[i])
        v, l = mp.mpf(rv[i]), mp.mpf(rl[i])
        F1, F2, H = er._FH(mp, par, t, v, l)
        f1, f2 = er._F(mp, par, t, v, l)
        h = er._H(mp, par, t, v, l)
        assert abs(H / h - 1) <= 1e-25
        assert abs(F1 - f1) <= 1e-25 * abs(v) and abs(F2 - f2) <= 1e-25
