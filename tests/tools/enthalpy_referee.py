"""Referees for the enthalpy of vaporization of a pure-component parameter row (CPU only).

Definition as in include/pcsaft_hip.h (pcs_pure_enthalpy_of_vaporization): at the saturated densities (rho_V, rho_L) of T,
    dh_vap [kJ/mol] = 1e-6 T [K] (1/rho_V - 1/rho_L) [m3/kmol] dp_sat/dT [Pa/K]                       (Clausius-Clapeyron)
                    = R T (-T [d(a/rho)/dT]_V + T [d(a/rho)/dT]_L + Z_V - Z_L),  Z = 1 - a/rho + a'   (direct form).

Two independent referees:

* ``cc_value`` -- the Clausius-Clapeyron form from the oracle alone: its VLE densities and column 8 (dp_sat/dT at fixed
  densities, which is the total slope: p_sat is stationary in both densities) of its vapour-pressure gradient.  prec / exact
  select the oracle's long-double or plain-double run; the GPU bars are ten times the discrepancy of the two.

* ``mp_value`` / ``mp_gradient`` -- mpmath, 50 digits, on critical_referee.helmholtz_mp (every class): the equilibrium by
  mp.findroot on (p_V - p_L, mu_V - mu_L) from the oracle's densities, the DIRECT form with mp.diff in T, and the exact total
  gradient w.r.t. (8 parameters, T) of that whole solve: the derivative of the root of F = 0 is -J^-1 dF/dx (implicit-function
  theorem, tangent form; every partial derivative a 50-digit central difference at relative step 1e-16, which costs a
  third of nested mp.diff calls and is exact to ~1e-18); ``mp_central_difference`` differentiates the solve itself --
  value at x + h and x - h, each with its own findroot -- and tests/test_enthalpy_referee.py holds the two together.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import critical_referee as cr  # noqa: E402

RHO_UNIT = cr.RHO_UNIT
R_KJ = 1.380649e-23 * 6.02214076e23 * 1e-3  # kJ/mol/K


def cc_value(orc, P, T, prec=1, exact=True):
    """-> dh [kJ/mol] (nan where the oracle finds no equilibrium), rho_v, rho_l [A^-3], failed [bool]."""
    P = np.ascontiguousarray(P, dtype=np.float64)
    T = np.ascontiguousarray(T, dtype=np.float64)
    rv, rl, st, _, _ = orc.pure_vle(P, T, prec=prec)
    st = np.asarray(st, dtype=bool) | ~np.isfinite(T) | ~(T > 0)
    ce = cr.packing_per_density(P, np.where(st, 300.0, T))
    sv, sl = np.where(st, 1e-3 / ce, rv), np.where(st, 0.4 / ce, rl)  # placeholder densities on rows that are not compared
    _, grad = orc.pure_property_grad("vapor_pressure", P, np.where(st, 300.0, T), None, sv, sl, exact=exact)
    dh = 1e-6 * T * (1.0 / sv - 1.0 / sl) * RHO_UNIT * grad[:, 8]
    return np.where(st, np.nan, dh), rv, rl, st


def cc_central_difference(orc, P, T, rel):
    """d dh / d(8 parameters, T) [n, 9] by four-point central differences of cc_value (long double) at relative step `rel`
    (zero columns where the parameter is zero: a row's class is not changed); nan where a displaced solve fails."""
    n = len(T)
    X = np.concatenate([P, T[:, None]], axis=1)
    out = np.zeros((n, 9))
    for k in range(9):
        h = rel * np.abs(X[:, k])
        if not h.any():
            continue
        v = []
        for f in (-2.0, -1.0, 1.0, 2.0):
            Y = X.copy()
            Y[:, k] += f * h
            v.append(cc_value(orc, np.ascontiguousarray(Y[:, :8]), np.ascontiguousarray(Y[:, 8]))[0])
        with np.errstate(invalid="ignore", divide="ignore"):
            out[:, k] = np.where(h > 0, (v[0] - 8.0 * v[1] + 8.0 * v[2] - v[3]) / (12.0 * h), 0.0)
    return out


# ---- mpmath ----------------------------------------------------------------------------------------------------------
def _a1(mp, par, T, rho):
    return mp.diff(lambda r: cr.helmholtz_mp(par, T, r), rho)


def _F(mp, par, T, rv, rl):
    """(p_V - p_L, mu_V - mu_L) in units of kT: p = rho - a + rho a', mu = ln rho + a'."""
    out = []
    for rho in (rv, rl):
        a, a1 = cr.helmholtz_mp(par, T, rho), _a1(mp, par, T, rho)
        out.append((rho - a + rho * a1, mp.log(rho) + a1))
    return out[0][0] - out[1][0], out[0][1] - out[1][1]


def _H(mp, par, T, rv, rl):
    """dh_vap / (R T), direct form."""
    h = []
    for rho in (rv, rl):
        at = mp.diff(lambda t: cr.helmholtz_mp(par, t, rho), T) / rho
        h.append(-T * at + 1 - cr.helmholtz_mp(par, T, rho) / rho + _a1(mp, par, T, rho))
    return h[0] - h[1]


def _solve(mp, par, T, rv0, rl0):
    return mp.findroot(lambda v, l: _F(mp, par, T, v, l), (mp.mpf(rv0), mp.mpf(rl0)), tol=mp.mpf(10) ** -35, maxsteps=60)


def _mpf_row(mp, par, T):
    return [mp.mpf(float(x)) for x in par], mp.mpf(float(T))


def mp_equilibrium(par, T, rv0, rl0):
    """Exact saturated densities (rho_V, rho_L) [A^-3] of one row at T from the start (rv0, rl0), as mpf."""
    mp = cr._mp()
    par, T = _mpf_row(mp, par, T)
    return tuple(_solve(mp, par, T, float(rv0), float(rl0)))


def mp_value(par, T, rv0, rl0):
    """Exact dh_vap [kJ/mol] of one row (direct form at the mpmath equilibrium) as mpf."""
    mp = cr._mp()
    par, T = _mpf_row(mp, par, T)
    rv, rl = _solve(mp, par, T, float(rv0), float(rl0))
    return mp.mpf(R_KJ) * T * _H(mp, par, T, rv, rl)


def _active(par):
    """directions in which the value depends on the parameter at all (critical_referee.mp_gradient has the same rule)"""
    keep = []
    for k in range(8):
        if k == 3 and par[3] == 0:
            continue
        if k in (4, 5, 6, 7) and (par[6] + par[7] == 0 or par[4] == 0):
            continue
        keep.append(k)
    return keep + [8]


def _with(par, T, k, x):
    if k == 8:
        return par, x
    th = list(par)
    th[k] = x
    return th, T


STEP = "1e-16"  # relative step of the gradient's central differences: truncation ~1e-32, rounding ~1e-34 at 50 digits


def _cd(mp, f, x):
    """central difference of a tuple-valued f at x (see STEP)"""
    h = abs(x) * mp.mpf(STEP)
    return [(p - m) / (2 * h) for p, m in zip(f(x + h), f(x - h))]


def _FH(mp, par, T, rv, rl):
    """(F1, F2, H) of _F and _H in one go, the inner derivatives (a' and a_T) by _cd: what mp_gradient differentiates.
    tests/test_enthalpy_referee.py holds it against the mp.diff forms."""
    F1 = F2 = H = 0
    for sign, rho in ((1, rv), (-1, rl)):
        a = cr.helmholtz_mp(par, T, rho)
        (a1,) = _cd(mp, lambda r: (cr.helmholtz_mp(par, T, r),), rho)
        (at,) = _cd(mp, lambda t: (cr.helmholtz_mp(par, t, rho),), T)
        F1 += sign * (rho - a + rho * a1)
        F2 += sign * (mp.log(rho) + a1)
        H += sign * (-T * at / rho + 1 - a / rho + a1)
    return F1, F2, H


def mp_gradient(par, T, rv0, rl0):
    """Exact d dh_vap [kJ/mol] / d(8 parameters, T) along the saturation line -> float array [9].  The site counts na, nb are
    differentiated as the continuous variables they are in the model."""
    mp = cr._mp()
    par, T = _mpf_row(mp, par, T)
    rv, rl = _solve(mp, par, T, float(rv0), float(rl0))
    dV = _cd(mp, lambda v: _FH(mp, par, T, v, rl), rv)  # d(F1, F2, H)/drho_V
    dL = _cd(mp, lambda l: _FH(mp, par, T, rv, l), rl)
    H = _FH(mp, par, T, rv, rl)[2]
    det = dV[0] * dL[1] - dL[0] * dV[1]
    out = np.zeros(9)
    for k in _active(par):
        dX = _cd(mp, lambda x: _FH(mp, *_with(par, T, k, x), rv, rl), T if k == 8 else par[k])
        dv = -(dL[1] * dX[0] - dL[0] * dX[1]) / det
        dl = -(dV[0] * dX[1] - dV[1] * dX[0]) / det
        dH = dX[2] + dV[2] * dv + dL[2] * dl
        out[k] = float(mp.mpf(R_KJ) * (T * dH + (H if k == 8 else 0)))
    return out


def mp_central_difference(par, T, rv0, rl0, rel=1e-10):
    """The same gradient by central differences of mp_value, every displaced value with its own equilibrium solve (50
    digits: a relative step of 1e-10 leaves a truncation error of ~1e-20 and no visible rounding) -> float array [9]."""
    mp = cr._mp()
    par_f, T_f = [float(x) for x in par], float(T)
    mpar, mT = _mpf_row(mp, par_f, T_f)
    out = np.zeros(9)
    for k in _active(mpar):
        x0 = mT if k == 8 else mpar[k]
        h = abs(x0) * mp.mpf(rel)
        v = []
        for s in (1, -1):
            th, t = _with(mpar, mT, k, x0 + s * h)
            rv, rl = _solve(mp, th, t, float(rv0), float(rl0))
            v.append(mp.mpf(R_KJ) * t * _H(mp, th, t, rv, rl))
        out[k] = float((v[0] - v[1]) / (2 * h))
    return out


# ---- the rows the tests share ------------------------------------------------------------------------------------------
REFEREE_THETA = (0.6, 0.9, 0.99)


def referee_rows(per_class=2, seed=31):
    """per_class parameter rows of each of the four classes (critical_referee.sample) -> [4 per_class, 8]"""
    P = cr.sample(400, seed=seed)
    cls = (P[:, 3] != 0).astype(np.int64) + 2 * (P[:, 4] != 0).astype(np.int64)
    return np.concatenate([P[cls == c][:per_class] for c in range(4)])
