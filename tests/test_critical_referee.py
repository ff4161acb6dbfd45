"""CPU: the two referees of the critical point (tests/tools/critical_referee.py) agree with each other, and the points they
return are ends of the vapour-liquid region as the oracle's own VLE solve sees it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import critical_referee as cr  # noqa: E402


@pytest.fixture(scope="module")
def mp_rows(oracle):
    P = cr.sample(60, seed=cr.MP_SEED, mu_zero=True)
    Tc, pc, rc, rr = cr.oracle_scan(oracle, P)
    exact = [cr.mp_critical(P[i], Tc[i], rr[i]) for i in range(len(P))]
    return P, (Tc, pc, rc, rr), exact


def test_mp_model_equals_the_vapour_pressure_referee_model():
    """helmholtz_mp (mpf parameters, all classes) is the model of mp_pure_check.helmholtz on mu = 0 rows."""
    import mp_pure_check as chk

    mp = cr._mp()
    P = cr.sample(12, seed=3, mu_zero=True)
    for par in P:
        T = 1.2 * par[2]
        rho = 0.2 / float(cr.packing_per_density(par[None, :], np.array([T]))[0])
        a = chk.helmholtz(par, T, rho)
        b = cr.helmholtz_mp([mp.mpf(float(x)) for x in par], T, rho)
        assert abs(a - b) <= abs(a) * mp.mpf(10) ** -40


def test_scan_agrees_with_mpmath_on_mu_zero_rows(mp_rows):
    P, (Tc, pc, rc, rr), exact = mp_rows
    assoc = P[:, 4] != 0
    assert assoc.any() and (~assoc).any()
    e = np.array([[abs(Tc[i] / float(T) - 1), abs(pc[i] / float(p) - 1), abs(rr[i] / float(rho) - 1)]
                  for i, (T, p, rho, _) in enumerate(exact)])
    print("scan vs mpmath, max rel: T_c %.3e p_c %.3e rho_c %.3e" % tuple(e.max(axis=0)))
    assert e[:, 0].max() <= cr.SCAN_TC_RESOLUTION
    assert e[:, 1].max() <= cr.SCAN_PC_RESOLUTION
    assert e[:, 2].max() <= cr.SCAN_RHO_RESOLUTION


def test_third_pressure_derivative_is_positive(mp_rows):
    _, _, exact = mp_rows
    assert all(p3 > 0 for _, _, _, p3 in exact)


def test_mp_referee_covers_polar_rows(oracle):
    """The dipole term of helmholtz_mp against the oracle scan (which knows nothing of it) on polar rows."""
    P = cr.sample(12, seed=5, mu_zero=False)
    Tc, pc, rc, rr = cr.oracle_scan(oracle, P)
    for i in range(len(P)):
        T, p, rho, p3 = cr.mp_critical(P[i], Tc[i], rr[i])
        assert p3 > 0
        assert abs(Tc[i] / float(T) - 1) <= cr.SCAN_TC_RESOLUTION and abs(pc[i] / float(p) - 1) <= cr.SCAN_PC_RESOLUTION
        assert abs(rr[i] / float(rho) - 1) <= cr.SCAN_RHO_RESOLUTION


def test_oracle_vle_exists_below_and_not_above(oracle):
    """The sample the GPU consistency test uses: the oracle ALONE solves every row at F_SUB T_c, with
    rho_V < rho_c < rho_L and p_sat < p_c, and no row at 1.03 T_c."""
    P = cr.vle_sample()
    polar, assoc = P[:, 3] != 0, P[:, 4] != 0
    for a in (False, True):
        for b in (False, True):
            assert ((polar == a) & (assoc == b)).sum() >= 50
    Tc, pc, rc, rr = cr.oracle_scan(oracle, P)
    rv, rl, st, _, _ = oracle.pure_vle(P, cr.F_SUB * Tc, prec=1)
    assert not st.any(), np.where(st)[0]
    assert (rv < rr).all() and (rr < rl).all()
    ps, st = oracle.pure_vapor_pressure(P, cr.F_SUB * Tc, prec=1)
    assert not st.any() and (ps < pc).all() and (ps > 0).all()
    _, _, st, _, _ = oracle.pure_vle(P, 1.03 * Tc, prec=1)
    assert st.all(), np.where(~st)[0]


def test_no_unstable_state_above_the_critical_temperature(oracle):
    """What the choice among several critical points rests on (csrc/pure_critical.hpp): above T_c the isotherms are
    mechanically stable at every density, 0.01 <= eta <= 0.7."""
    P = cr.vle_sample()
    Tc, _, _, _ = cr.oracle_scan(oracle, P)
    eta = np.linspace(0.01, 0.7, 140)
    for f in (1.05, 1.5, 3.0):
        T = f * Tc
        rho = eta[None, :] / cr.packing_per_density(P, T)[:, None]
        dp = oracle.pure_derivatives(np.repeat(P, len(eta), axis=0), np.repeat(T, len(eta)), rho.ravel())[2]
        assert (dp > 0).all(), f
