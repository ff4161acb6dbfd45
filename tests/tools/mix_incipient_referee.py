"""Referee for the gradient of the incipient-phase composition of a binary bubble / dew point (test infrastructure, numpy only).

y = mole fraction of component 1 in the incipient phase (vapour for bubble, liquid for dew) of the rho4 that
oracle.pyoracle.mix_bubble_dew(..., prec=1) returns (long-double solve).  The oracle has no exact dy/dtheta, so the referee
is Richardson-extrapolated central differences of that solve in each of the 19 directions (16 parameters, kij0, kij1, T):
    D(h) = [f(theta_k (1 + h)) - f(theta_k (1 - h))] / (2 h theta_k),     R = (4 D(h) - D(2 h)) / 3     (O(h^4)),
every displaced solve started from the base pressure.  A direction whose parameter is zero has no relative step and is not
checked (mask `checked`): a zero dipole moment, the association parameters of a component without sites, kij1 = 0 (which
selects the combining rule) -- moving any of them away from zero would change the model class, not displace the row.
The same machinery on f = p gives a second block that the oracle's exact mix_bubble_dew_grad(exact=True) measures.

Error of the referee, per row and relative to the row's largest checked component: est = max_k |R_k - D_k(h)| / max_k |R_k|
(the whole h^2 term of the plain difference, a generous bound for R) and, independently, the p block against the exact
gradient (e, tests/test_mix_incipient_referee.py).

Input set: tests/tools/mix_temperature_referee.py's `inputs` (192 parameter rows x 3 temperature factors, both problems).  A row
is dropped in advance, by the oracle alone, when that set drops it, when a displaced solve fails or lands on another branch
(|dy| > JUMP or |d ln p| > JUMP: with |d ln f / d ln theta| <= 50 on this set a displacement of 2 h moves either by < 1e-3),
or when est of the y block exceeds BAR_FLOOR -- the floor of the GPU test's bar max(10 e, BAR_FLOOR), so no row above the bar
is ever kept.  At most CAP of a (class, factor, problem) cell may be dropped; the committed H meets that.

H: rounding puts eps / h ~ 4e-11 into D(h) (p and y come back as doubles) and the h^2 term of D(h) is 1.5e-12 times the
third logarithmic derivative.  Measured on the oracle alone (tests/test_mix_incipient_referee.py prints them): with H = 3e-6
the largest dropped share of a cell is 3/32 for both problems (bubble: the set's own drops only; dew: 6 rows by est), and
e = 2.5e-8 (bubble) / 9.5e-9 (dew).  H = 1e-5 has the smaller e (4.7e-9 / 1.5e-9, the rounding term) but drops 4/32 of one
dew cell by est; H = 1e-6 gains nothing on e.
"""
import numpy as np

import mix_temperature_referee as tref

H = 3e-6
JUMP = 1e-2
BAR_FLOOR = 1e-8  # the bar tests/test_dilute_gpu.py applies to pcs_mix_jacobian
CAP = 0.10
N_DIRS = 19


def molefrac(rho4, dew, component=0):
    inc = rho4[:, 2:4] if dew else rho4[:, 0:2]
    return inc[:, component] / (inc[:, 0] + inc[:, 1])


def theta(P, K, T):
    """[n,19] = (16 parameters, kij0, kij1, T)"""
    return np.concatenate((P.reshape(len(T), 16), K, T[:, None]), axis=1)


def _split(th):
    return np.ascontiguousarray(th[:, :16].reshape(-1, 2, 8)), np.ascontiguousarray(th[:, 16:18]), np.ascontiguousarray(th[:, 18])


def richardson(orc, P, K, T, z, p_base, y_base, dew, h=None):
    """-> dict(Rp, Dp, Ry, Dy [n,19] (NaN where not checked or failed), checked [n,19] bool, bad [n] bool = a displaced solve
    failed or jumped).  y is differenced through the SMALLER of the two mole fractions (dy_1 = -dy_2 exactly): next to a pure
    incipient phase y_1 = 1 - 1e-10 as a double has lost the digits its own differences need, y_2 has not."""
    h = H if h is None else h
    n = len(T)
    th0 = theta(P, K, T)
    checked = th0 != 0.0
    out = {k: np.full((n, N_DIRS), np.nan) for k in ("Rp", "Dp", "Ry", "Dy")}
    bad = np.zeros(n, dtype=bool)
    for k in range(N_DIRS):
        rows = np.nonzero(checked[:, k])[0]
        if len(rows) == 0:
            continue
        f = {}
        for s in (-2, -1, 1, 2):
            th = th0[rows].copy()
            th[:, k] *= 1.0 + s * h
            Pk, Kk, Tk = _split(th)
            p, rho4, st = orc.mix_bubble_dew(Pk, Kk, Tk, z[rows], p_base[rows], dew, prec=1)
            with np.errstate(invalid="ignore", divide="ignore"):
                y = molefrac(rho4, dew)
                jump = ~(np.abs(y - y_base[rows]) < JUMP) | ~(np.abs(np.log(p / p_base[rows])) < JUMP)
                y = np.where(y_base[rows] <= 0.5, y, -molefrac(rho4, dew, 1))
            bad[rows[st | jump]] = True
            f[s] = (p, y)
        step = h * th0[rows, k]
        for j, (kr, kd) in enumerate((("Rp", "Dp"), ("Ry", "Dy"))):
            d1 = (f[1][j] - f[-1][j]) / (2.0 * step)
            d2 = (f[2][j] - f[-2][j]) / (4.0 * step)
            out[kd][rows, k] = d1
            out[kr][rows, k] = (4.0 * d1 - d2) / 3.0
    out["checked"], out["bad"] = checked, bad
    return out


def row_error(got, want, checked):
    """[n]: max_k |got - want| over the checked directions, relative to the row's largest checked |want|"""
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.where(checked, np.abs(got - want), 0.0)
        return np.nanmax(d, axis=1) / np.nanmax(np.where(checked, np.abs(want), 0.0), axis=1)


def quotient(Jp, Jy):
    """the two blocks [n,19] w.r.t. (.., T) at fixed T -> dy/d(16 parameters, kij0, kij1, p_spec) along p(theta, T) = p_spec"""
    dy_dp = Jy[:, 18:19] / Jp[:, 18:19]
    return np.concatenate((Jy[:, :18] - dy_dp * Jp[:, :18], dy_dp), axis=1)


_CACHE = {}


def _spread(n, idx, a, fill):
    """rows idx of a [n, ...] array filled with `fill`"""
    out = np.full((n,) + a.shape[1:], fill, dtype=a.dtype)
    out[idx] = a
    return out


def inputs(orc, dew):
    """The temperature referee's input set of one problem (its fields, untouched) with the Richardson blocks, the kept rows
    and the bar.  Cached per process."""
    if dew in _CACHE:
        return _CACHE[dew]
    c = tref.Inputs()
    c.__dict__.update(tref.inputs(orc, dew).__dict__)
    idx = np.nonzero(c.keep)[0]
    c.y = _spread(c.n, idx, molefrac(c.rho4[idx], dew), np.nan)
    r = richardson(orc, c.P[idx], c.K[idx], c.T[idx], c.z[idx], c.p_spec[idx], c.y[idx], dew)
    c.Rp, c.Dp, c.Ry, c.Dy = (_spread(c.n, idx, r[k], np.nan) for k in ("Rp", "Dp", "Ry", "Dy"))
    c.checked = _spread(c.n, idx, r["checked"], False)
    c.fd_bad = _spread(c.n, idx, r["bad"], True)
    c.est_y = row_error(c.Dy, c.Ry, c.checked)
    c.est_p = row_error(c.Dp, c.Rp, c.checked)
    with np.errstate(invalid="ignore"):
        c.keep_y = c.keep & ~c.fd_bad & (c.est_y <= BAR_FLOOR)
    # the p block against the oracle's exact gradient: the referee's error measured independently
    c.err_p = row_error(c.Rp, c.grad, c.checked)
    c.e = float(np.max(c.err_p[c.keep_y])) if c.keep_y.any() else np.inf
    c.bar = max(10.0 * c.e, BAR_FLOOR)
    c.dropped_share_y = np.array([np.mean(~c.keep_y[c.cell == k]) for k in np.unique(c.cell)])
    _CACHE[dew] = c
    return c
