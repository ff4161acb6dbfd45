"""Exact referee for the two gradient blocks of a binary bubble / dew point (test infrastructure, numpy only).

The blocks are dp/dtheta [Pa] and dy/dtheta (y = mole fraction of component 1 in the incipient phase) w.r.t. theta = (16
parameters, k_ij, eps_AiBj, T), the 19 columns pcs_mix_jacobian and pcs_mix_point_jacobian write.  They are assembled on the host
by the implicit-function theorem from oracle.mix_derivatives_vjp_exact alone (nested long-double duals, every column seeded, tied
to the reference's autograd by tests/test_oracle_state_grad.py): three calls per phase, upstreams gp = 1, gmu = (1, 0) and
gmu = (0, 1), give the theta- and rho-derivatives of p, mu_0 and mu_1 (reduced).  S = the specified phase (liquid for bubble,
vapour for dew), I = the incipient one, v = (rho_S total at fixed z, rho_I0, rho_I1):

    F = (ln rho_S0 + mu_0^S - ln rho_I0 - mu_0^I,  the same for component 1,  p^S - p^I)
    dv/dtheta  = -J^-1 dF/dtheta,     J = dF/dv  (3 x 3; solved for d ln v, rows equilibrated, partial pivoting)
    dy0/dtheta = (rho_I1 drho_I0/dtheta - rho_I0 drho_I1/dtheta) / (rho_I0 + rho_I1)^2
    dp/dtheta  = kB/A^3 T (dp_red^V/dtheta + dp_red^V/drho^V . drho^V/dtheta) + [theta = T] kB/A^3 p_red^V

prec=1: the oracle in long double and the assembly in numpy.longdouble -- the referee.  prec=0: the oracle in double and the same
assembly in float64 -- the fp64 twin, the yardstick for what fp64 can deliver on a row.  A column whose parameter is zero carries
the derivative of the formula that the row's real parts select (the oracle's convention: eps_AiBj = 0 keeps the mean combining
rule, that column is 0; kappa_ab, eps_ab, na, nb of a site-less component next to an associating one are not 0).

Input set: tests/tools/mix_temperature_referee.py's `inputs` (192 parameter rows x 3 temperature factors, 6 classes, both
problems), blocks at the oracle's rho4 on its kept rows.  e_row = twin against referee, relative to the row's largest exact
component; bar_row = max(BAR_FLOOR, 10 e_row), tight = (bar_row == BAR_FLOOR), separately for p and y.
"""
import numpy as np

import mix_temperature_referee as tref

P_UNIT = 1.380649e-23 / 1e-30  # kB / A^3: reduced pressure x T -> Pa
BAR_FLOOR = 1e-10
N_DIRS = 19
COLUMNS = tuple("%s_%d" % (s, c) for c in (1, 2) for s in ("m", "sigma", "eps_k", "mu", "kappa_ab", "eps_ab", "na", "nb")) + (
    "k_ij", "eps_AiBj", "T")


def theta(P, K, T):
    """[n,19] = (16 parameters, k_ij, eps_AiBj, T)"""
    return np.concatenate((P.reshape(len(T), 16), K, T[:, None]), axis=1)


def solve3(J, B):
    """x [n,3,m] with J x = B (J [n,3,3], B [n,3,m]) in the dtype of J: rows scaled by their largest entry, Gaussian elimination
    with partial pivoting, vectorised over the rows of the batch."""
    n = J.shape[0]
    A = np.concatenate((J, B), axis=2)
    A = A / np.abs(J).max(axis=2)[:, :, None]
    i = np.arange(n)
    for k in range(2):
        piv = k + np.argmax(np.abs(A[:, k:, k]), axis=1)
        top, low = A[i, k].copy(), A[i, piv].copy()
        A[i, piv], A[i, k] = top, low
        for r in range(k + 1, 3):
            A[:, r] = A[:, r] - (A[:, r, k] / A[:, k, k])[:, None] * A[:, k]
    x = np.empty_like(B)
    x[:, 2] = A[:, 2, 3:] / A[:, 2, 2:3]
    x[:, 1] = (A[:, 1, 3:] - A[:, 1, 2:3] * x[:, 2]) / A[:, 1, 1:2]
    x[:, 0] = (A[:, 0, 3:] - A[:, 0, 1:2] * x[:, 1] - A[:, 0, 2:3] * x[:, 2]) / A[:, 0, 0:1]
    return x


def _phase(orc, P, K, T, rho, prec, dt):
    """-> G [n,3,21]: rows (mu_0, mu_1, p), columns (19 directions, rho_0, rho_1) of one phase; p_red [n]"""
    n = len(T)
    o, z, z2 = np.ones(n), np.zeros(n), np.zeros((n, 2))
    e0, e1 = np.tile([1.0, 0.0], (n, 1)), np.tile([0.0, 1.0], (n, 1))
    G = np.stack([orc.mix_derivatives_vjp_exact(P, K, T, rho, z, gp, gmu, z2, prec=prec) for gp, gmu in ((z, e0), (z, e1), (o, z2))], axis=1)
    p = orc.mix_derivatives_exact(P, K, T, rho)[1] if prec else orc.mix_derivatives(P, K, T, rho, robust=True)[1]
    return G.astype(dt), p.astype(dt)


def blocks(orc, P, K, T, rho4, dew, prec=1):
    """(Jp [n,19] in Pa per unit of theta, Jy [n,19]) at the densities rho4 = (rhoV_1, rhoV_2, rhoL_1, rhoL_2), as doubles."""
    dt = np.longdouble if prec else np.float64
    P, K, T, rho4 = (np.ascontiguousarray(x, dtype=np.float64) for x in (P, K, T, rho4))
    n = len(T)
    V, L = rho4[:, 0:2], rho4[:, 2:4]
    S, I = (V, L) if dew else (L, V)
    GS, pS = _phase(orc, P, K, T, np.ascontiguousarray(S), prec, dt)
    GI, pI = _phase(orc, P, K, T, np.ascontiguousarray(I), prec, dt)
    S, I, Tl = S.astype(dt), I.astype(dt), T.astype(dt)
    rS = S[:, 0] + S[:, 1]
    z = S / rS[:, None]
    J = np.empty((n, 3, 3), dtype=dt)
    J[:, :, 0] = GS[:, :, 19] * z[:, 0:1] + GS[:, :, 20] * z[:, 1:2]
    J[:, 0:2, 0] += (1 / rS)[:, None]
    J[:, :, 1:3] = -GI[:, :, 19:21]
    J[:, 0, 1] -= 1 / I[:, 0]
    J[:, 1, 2] -= 1 / I[:, 1]
    # solved for d ln v: the columns scaled by the densities, which span 1e-26 ... 1e-2 A^-3 at a dew point far below T_c
    scale = np.stack((rS, I[:, 0], I[:, 1]), axis=1)
    dv = solve3(J * scale[:, None, :], -(GS[:, :, :N_DIRS] - GI[:, :, :N_DIRS])) * scale[:, :, None]  # [n,3,19]: dv/dtheta
    rI = I[:, 0] + I[:, 1]
    Jy = (I[:, 1:2] * dv[:, 1] - I[:, 0:1] * dv[:, 2]) / (rI * rI)[:, None]
    if dew:  # the vapour is the specified phase: drho^V = z drho_S
        dpV = GS[:, 2, :N_DIRS] + J[:, 2, 0:1] * dv[:, 0]
        pV = pS
    else:
        dpV = GI[:, 2, :N_DIRS] + GI[:, 2, 19:20] * dv[:, 1] + GI[:, 2, 20:21] * dv[:, 2]
        pV = pI
    Jp = dt(P_UNIT) * Tl[:, None] * dpV
    Jp[:, 18] += dt(P_UNIT) * pV
    return Jp.astype(np.float64), Jy.astype(np.float64)


def row_error(got, want):
    """[n]: max_k |got - want| over all 19 columns, relative to the row's largest |want|"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)


def column_error(got, want, rows):
    """[19]: max_i |got - want| / max_i |want| over the rows `rows` (0 where the exact column is identically zero there)"""
    d, w = np.abs(got[rows] - want[rows]).max(axis=0), np.abs(want[rows]).max(axis=0)
    return np.where(w > 0, d / np.where(w > 0, w, 1.0), 0.0)


def spread(n, idx, a, fill=np.nan):
    """rows idx of a [n, ...] array filled with `fill`"""
    out = np.full((n,) + a.shape[1:], fill, dtype=a.dtype)
    out[idx] = a
    return out


_CACHE = {}


def inputs(orc, dew):
    """The temperature referee's input set of one problem (its fields, untouched) with, on its kept rows (NaN elsewhere):
    Jp, Jy exact blocks; Jp64, Jy64 the fp64 twin's; e_p, e_y, bar_p, bar_y [n]; tight_p, tight_y [n] bool (False off the kept
    rows); theta [n,19]; zero_param [n,19] = theta == 0; zero_entry_p / zero_entry_y [n,19] = the parameter is 0 and the exact
    derivative is not; full_rows[cls] = the kept rows of the class on which every column the class uses (a column whose
    parameter is non-zero on some row of the class) has a non-zero parameter; zero_rows[cls][k] = its kept rows whose
    parameter of the column k is 0, for every column k the class uses or fills.  Cached per process."""
    if dew in _CACHE:
        return _CACHE[dew]
    c = tref.Inputs()
    c.__dict__.update(tref.inputs(orc, dew).__dict__)
    idx = np.nonzero(c.keep)[0]
    a = (c.P[idx], c.K[idx], c.T[idx], c.rho4[idx], dew)
    c.Jp, c.Jy = (spread(c.n, idx, b) for b in blocks(orc, *a, prec=1))
    c.Jp64, c.Jy64 = (spread(c.n, idx, b) for b in blocks(orc, *a, prec=0))
    c.theta = theta(c.P, c.K, c.T)
    c.zero_param = c.theta == 0.0
    for s in "py":
        J, J64 = getattr(c, "J" + s), getattr(c, "J" + s + "64")
        e = row_error(J64, J)
        with np.errstate(invalid="ignore"):
            bar = np.maximum(BAR_FLOOR, 10.0 * e)
        setattr(c, "e_" + s, e)
        setattr(c, "bar_" + s, bar)
        setattr(c, "tight_" + s, c.keep & (bar == BAR_FLOOR))
        with np.errstate(invalid="ignore"):
            setattr(c, "zero_entry_" + s, c.keep[:, None] & c.zero_param & (J != 0.0))
    c.full_rows, c.zero_rows = {}, {}
    for k in range(tref.N_CLASSES):
        m = c.keep & (c.cls == k)
        used = (~c.zero_param[c.cls == k]).any(axis=0)
        c.full_rows[k] = m & ~c.zero_param[:, used].any(axis=1)
        filled = (c.zero_entry_p[m] | c.zero_entry_y[m]).any(axis=0)
        c.zero_rows[k] = {j: m & c.zero_param[:, j] for j in np.nonzero(used | filled)[0] if (m & c.zero_param[:, j]).any()}
    _CACHE[dew] = c
    return c
