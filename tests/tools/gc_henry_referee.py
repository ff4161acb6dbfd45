"""Referee and input set for GcPcSaftMix.henrys_law_constant (test infrastructure, numpy + oracle only).  It takes none of the
kernel's decisions.

Definition.  With s the solute of a row, v = 1 - s its solvent, rho_L the saturated liquid density of molecule v taken as a pure
fluid at T and mu_s = da/drho_s the residual chemical potential of the row's two-molecule model at the partial densities
rho_v = rho_L, rho_s = 0:
    ln H [Pa] = ln(rho_L T / P_RED) + mu_s,      P_RED = 1e-30 / k_B.
rho_L, rho_V, p_sat and the slope p'_L = dp/drho at the liquid root are the long-double solve of gc_saturation_referee (a
fixed-grid scan of the pure line and Newton on (p, mu)); mu_s is oracle.gc_derivatives(prec=1) at (rho_L e_v), long double
rounded to double on return.  The fp64 twin is the same with prec=0 for the solve and for mu_s; it sets the value bars.

Gradient.  At fixed T and for any parameter theta, with @ a partial derivative at fixed densities,
    d ln H/dtheta = @mu_s/@theta + dlnh_drho d rho_L/dtheta,      dlnh_drho = 1/rho_L + @mu_s/@rho_v,
and d ln H/dT has 1/T on top.  @mu_s/@rho_v is the density column 3 + v of oracle.gc_derivatives_vjp_exact with gmu[:, s] = 1.
For an upstream gradient g of ln H the gradient is that exact call's (row[:, :3], grad_seg, grad_kab) under gmu[:, s] = g, plus
gc_saturation_referee.gradient(..., g dlnh_drho, which=1) -- the gradient of rho_L under the weight g dlnh_drho -- plus g/T on T.

Input set (the GPU test uses the same): gc_saturation_referee.inputs(oracle), reused as it is.  Its row i has the component
c.comp[i] as the pure fluid the temperature was made for: that is the SOLVENT here, and the row's solute is 1 - c.comp[i].  For
solute s the rows are those with c.comp == 1 - s: the solvent's four temperature factors 0.55 .. 0.95 x T_top on the 384 rows
of every model class, 1,536 rows per solute; in the interleaved batch (gc_saturation_referee.interleave) the other half are wave
mates.  A row is kept when the saturation referee keeps it and ln H is finite; at most CAP of the rows of any (class, solute,
factor) cell may be dropped (tests/test_gc_henry_referee.py).
"""
import numpy as np

import gc_saturation_referee as sref

CAP = 0.10
P_RED = sref.P_RED
SEED = 2047
interleave = sref.interleave


class Inputs:
    pass


_CACHE = {}


def _r2(col, rho):
    out = np.zeros((len(rho), 2))
    out[np.arange(len(rho)), col] = rho
    return out


def mu_solute(m, idx, solute, T, rho_l, prec=1):
    """mu_s [n] at the partial densities rho_v = rho_l, rho_s = 0"""
    enc, phi = m.sub(idx)
    mu = m.orc.gc_derivatives(enc, phi, T, _r2(1 - solute, rho_l), robust=True, prec=prec)[2]
    return mu[np.arange(len(T)), solute]


def ln_h(T, rho_l, mu_s):
    return np.log(rho_l * T / P_RED) + mu_s


def exact_mu(m, idx, solute, T, rho_l, g):
    """gc_derivatives_vjp_exact at (rho_l e_v) with the weight g on mu_s alone -> grad_row [n,5], grad_seg [S,8], grad_kab [S,S]"""
    enc, phi = m.sub(idx)
    n = len(T)
    z, z2 = np.zeros(n), np.zeros((n, 2))
    return m.orc.gc_derivatives_vjp_exact(enc, phi, T, _r2(1 - solute, rho_l), z, z, _r2(solute, g), z2)


def dmu_drho(m, idx, solute, T, rho_l):
    """@mu_s/@rho_v [n]"""
    n = len(T)
    return exact_mu(m, idx, solute, T, rho_l, np.ones(n))[0][np.arange(n), 3 + (1 - solute)]


def solve(m, idx, solute, T, prec=1):
    """Henry constants of the rows idx of m from scratch (the saturation referee's solve on the solvent, then mu_s):
    dict(ok, ln_h, rho_v, rho_l, p_sat, mu_s); NaN where not ok"""
    idx, solute, T = np.asarray(idx), np.asarray(solute), np.asarray(T, dtype=np.float64)
    s = sref.solve(m, idx, 1 - solute, T, prec)
    out = {"ok": s["ok"].copy(), "rho_v": s["rho_v"], "rho_l": s["rho_l"], "p_sat": s["p_sat"],
           "mu_s": np.full(len(T), np.nan), "ln_h": np.full(len(T), np.nan)}
    k = np.nonzero(s["ok"])[0]
    if len(k):
        out["mu_s"][k] = mu_solute(m, idx[k], solute[k], T[k], s["rho_l"][k], prec)
        out["ln_h"][k] = ln_h(T[k], s["rho_l"][k], out["mu_s"][k])
    out["ok"] &= np.isfinite(out["ln_h"])
    return out


def gradient(m, idx, solute, T, rho_v, rho_l, p_sat, dp_l, dlnh, g):
    """The formulas of the module docstring for an upstream gradient g [n] of ln H:
    -> row [n,3] = g d ln H / d(phi_0, phi_1, T), grad_seg [S,8], grad_kab [S,S] (the sums over the rows)."""
    row_m, seg_m, kab_m = exact_mu(m, idx, solute, T, rho_l, g)
    row_r, seg_r, kab_r = sref.gradient(m, idx, 1 - solute, T, rho_v, rho_l, p_sat, dp_l, g * dlnh, 1)
    row = row_m[:, :3] + row_r
    row[:, 2] += g / T
    return row, seg_m + seg_r, kab_m + kab_r


def inputs(orc):
    """The saturation referee's input set with the Henry constant of every row's other molecule: arrays over its 3,072 rows."""
    if "inputs" in _CACHE:
        return _CACHE["inputs"]
    c = sref.inputs(orc)
    h = Inputs()
    h.c, h.m, h.n = c, c.m, c.n
    h.solute = 1 - c.comp
    nan = lambda: np.full(c.n, np.nan)
    h.mu_s, h.mu_s64, h.ln_h, h.ln_h64, h.dmu, h.dlnh = nan(), nan(), nan(), nan(), nan(), nan()
    k = np.nonzero(c.keep)[0]
    h.mu_s[k] = mu_solute(c.m, c.row[k], h.solute[k], c.T[k], c.rho_l[k])
    h.ln_h[k] = ln_h(c.T[k], c.rho_l[k], h.mu_s[k])
    h.dmu[k] = dmu_drho(c.m, c.row[k], h.solute[k], c.T[k], c.rho_l[k])
    h.dlnh[k] = 1.0 / c.rho_l[k] + h.dmu[k]
    k2 = np.nonzero(c.keep & c.twin["ok"])[0]
    h.mu_s64[k2] = mu_solute(c.m, c.row[k2], h.solute[k2], c.T[k2], c.twin["rho_l"][k2], prec=0)
    h.ln_h64[k2] = ln_h(c.T[k2], c.twin["rho_l"][k2], h.mu_s64[k2])
    h.keep = c.keep & np.isfinite(h.ln_h) & np.isfinite(h.dlnh)
    h.cell, h.cells = c.cell, c.cells  # (class, solvent = 1 - solute, factor)
    h.dropped_share = {int(q): float(np.mean(~h.keep[h.cell == q])) for q in h.cells}
    with np.errstate(invalid="ignore"):
        h.twin_lnh = np.where(h.keep, np.abs(h.ln_h64 - h.ln_h), np.nan)  # absolute: ln H is a logarithm
    for val in vars(h).values():
        if isinstance(val, np.ndarray):
            val.setflags(write=False)
    _CACHE["inputs"] = h
    return h


def weighted(orc, h, solute):
    """The referee of the gradient test, once per solute: seeded upstream gradients g ~ U(0.5, 1.5) of ln H on the kept rows of the
    solute, and per model class (the weights masked to it) the gradient sums: {'g': [n], 'groups': {class: dict(rows, row [m,3],
    grad_kab, grad_seg)}, 'all': sums over the classes}."""
    key = ("weighted", solute)
    if key not in _CACHE:
        c = h.c
        mine = h.keep & (h.solute == solute)
        g = np.where(mine, np.random.default_rng(SEED + solute).uniform(0.5, 1.5, c.n), 0.0)
        out = {"g": g, "groups": {}}
        S = c.m.enc["S"]
        tot = {"grad_kab": np.zeros((S, S)), "grad_seg": np.zeros((S, 8))}
        for k in c.classes:
            rows = np.nonzero(mine & (c.cls == k))[0]
            if len(rows) == 0:
                continue
            row, gseg, gkab = gradient(c.m, c.row[rows], h.solute[rows], c.T[rows], c.rho_v[rows], c.rho_l[rows], c.p_sat[rows],
                                       c.dp_l[rows], h.dlnh[rows], g[rows])
            out["groups"][int(k)] = {"rows": rows, "row": row, "grad_kab": gkab, "grad_seg": gseg}
            tot["grad_kab"] += gkab
            tot["grad_seg"] += gseg
        out["all"] = tot
        _CACHE[key] = out
    return _CACHE[key]
