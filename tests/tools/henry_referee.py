"""Referee for Henry's law constants of binary-mixture rows (CPU only; include/pcsaft_hip.h, pcs_mix_henry).

With s the solute, v the solvent, rho_L the saturated liquid density of the pure solvent at T and mu_s the solute's residual
chemical potential at the partial densities (rho_v, rho_s) = (rho_L, 0):

    ln H [Pa] = ln(rho_L [A^-3] T KT_A3) + mu_s

Everything comes from the oracle: ``pure_vle`` on the solvent row, ``mix_derivatives_exact`` at (rho_L, 0), and for the
gradient w.r.t. (16 parameters, k_ij, eps_AiBj, T) the chain rule

    d ln H / dx = [d mu_s / dx]_rho + (1 / rho_L + d mu_s / d rho_v) d rho_L / dx + [x = T] / T,

the first term and d mu_s / d rho_v from ``mix_derivatives_vjp_exact`` with the weight 1 on mu_s, and d rho_L / d(theta_v, T),
the TOTAL derivative of the saturated liquid density, from ``pure_property_grad("equilibrium_liquid_density", exact=True)``:
that is the gradient at fixed densities of  rho_L - (p(rho_L) - p*) / p'(rho_L)  [kmol/m3] with the equal-area pressure p*,
which at the converged equilibrium IS the total derivative (p* is stationary in both densities, and the Newton quotient
carries the response of the liquid root to p*); tests/test_henry_referee.py holds it against central differences of the solve.

``prec=1`` is the referee (long double, rounded to double on return); ``prec=0`` is its twin, the same formulas on the
oracle's plain-double entries.  The distance of the two is what fp64 can deliver on a row and sets the bars of the GPU tests.
"""
import numpy as np

KT_A3 = 1.380649e-23 * 1e30  # p [Pa] = reduced p [A^-3] * KT_A3 * T [K]
RHO_UNIT = 1e3 * (6.02214076e23 * 1e-30)  # rho [A^-3] = RHO_UNIT * rho [kmol/m3]


def _sides(solute):
    if solute not in (0, 1):
        raise ValueError("solute must be 0 or 1")
    return solute, 1 - solute


def _rho2(rl, s):
    rho = np.zeros((len(rl), 2))
    rho[:, 1 - s] = rl
    return rho


def value(orc, par, kij, T, solute, prec=1):
    """-> dict(lnh [n], rho_v, rho_l [A^-3] of the pure solvent, mu [n] = mu_s, failed [bool]); nan in failed rows."""
    s, v = _sides(solute)
    par = np.ascontiguousarray(par, dtype=np.float64)
    kij = np.ascontiguousarray(kij, dtype=np.float64)
    T = np.ascontiguousarray(T, dtype=np.float64)
    rv, rl, st, _, _ = orc.pure_vle(np.ascontiguousarray(par[:, v, :]), T, prec=prec)
    st = np.asarray(st, dtype=bool)
    rl_safe = np.where(st, 1e-2, rl)  # placeholder density on rows that are not compared
    if prec == 1:
        mu = orc.mix_derivatives_exact(par, kij, T, _rho2(rl_safe, s))[2][:, s]
    else:
        mu = orc.mix_derivatives(par, kij, T, _rho2(rl_safe, s), robust=True)[2][:, s]
    with np.errstate(invalid="ignore", divide="ignore"):
        lnh = np.log(rl_safe * T * KT_A3) + mu
    st = st | ~np.isfinite(lnh)
    nan = lambda x: np.where(st, np.nan, x)
    return {"lnh": nan(lnh), "rho_v": nan(rv), "rho_l": nan(rl), "mu": nan(mu), "failed": st}


def drho_l(orc, par_v, T, rho_v, rho_l, prec=1):
    """Total derivative of the saturated liquid density [A^-3] w.r.t. (8 parameters, T) -> [n, 9]."""
    _, grad = orc.pure_property_grad("equilibrium_liquid_density", par_v, T, None, rho_v, rho_l, exact=(prec == 1))
    return RHO_UNIT * grad[:, :9]  # the property's value is in kmol/m3


def gradient(orc, par, kij, T, solute, prec=1, val=None):
    """-> (d ln H / d(16 parameters, k_ij, eps_AiBj, T) [n, 19], dlnh_drho [n] = 1 / rho_L + d mu_s / d rho_v); nan in the
    rows that `value` fails."""
    s, v = _sides(solute)
    par = np.ascontiguousarray(par, dtype=np.float64)
    kij = np.ascontiguousarray(kij, dtype=np.float64)
    T = np.ascontiguousarray(T, dtype=np.float64)
    n = len(T)
    val = value(orc, par, kij, T, solute, prec) if val is None else val
    st = val["failed"]
    rl = np.where(st, 1e-2, val["rho_l"])
    rvap = np.where(st, 1e-6, val["rho_v"])
    gmu = np.zeros((n, 2))
    gmu[:, s] = 1.0
    zero = np.zeros(n)
    G = orc.mix_derivatives_vjp_exact(par, kij, T, _rho2(rl, s), zero, zero, gmu, np.zeros((n, 2)), prec=prec)
    w = 1.0 / rl + G[:, 19 + v]
    dr = drho_l(orc, np.ascontiguousarray(par[:, v, :]), T, rvap, rl, prec)
    out = G[:, :19].copy()
    out[:, 8 * v:8 * v + 8] += w[:, None] * dr[:, :8]
    out[:, 18] += w * dr[:, 8] + 1.0 / T
    out[st] = np.nan
    return out, np.where(st, np.nan, w)


def reference(orc, par, kij, T, solute):
    """Referee and twin in one go -> dict(lnh, grad, rho_v, rho_l, failed: the referee's; d_lnh [n], d_grad [n] = |twin -
    referee| of ln H and of the gradient (largest component, relative to the row's largest referee component), d_w [n] = the
    same, relative, of dlnh_drho; inf where the twin fails a row the referee solves)."""
    a = value(orc, par, kij, T, solute, 1)
    b = value(orc, par, kij, T, solute, 0)
    ga, wa = gradient(orc, par, kij, T, solute, 1, a)
    gb, wb = gradient(orc, par, kij, T, solute, 0, b)
    with np.errstate(invalid="ignore"):
        d_lnh = np.abs(b["lnh"] - a["lnh"])
        d_grad = np.abs(gb - ga).max(axis=1) / np.abs(ga).max(axis=1)
        d_w = np.abs(wb / wa - 1.0)
    only_twin = b["failed"] & ~a["failed"]
    for d in (d_lnh, d_grad, d_w):
        d[only_twin] = np.inf
    return {"lnh": a["lnh"], "grad": ga, "dlnh_drho": wa, "rho_v": a["rho_v"], "rho_l": a["rho_l"], "failed": a["failed"],
            "d_lnh": d_lnh, "d_grad": d_grad, "d_w": d_w}
