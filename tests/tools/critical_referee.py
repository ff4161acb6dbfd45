"""Referees for the vapour-liquid critical point of a pure-component parameter row (CPU only).

Definitions as in include/pcsaft_hip.h (pcs_pure_critical_point): with the reduced residual Helmholtz energy density
a(T, rho), p/kT = rho - a + rho a', the critical point is the state with p_rho/kT = 1 + rho a'' = 0 and
p_rhorho/kT = a'' + rho a''' = 0 (p_rhorhorho > 0) at the end of the vapour-liquid loop.

Two independent referees:

* ``mp_critical`` / ``mp_gradient`` -- mpmath, 50 digits, on the Helmholtz energy of tests/tools/mp_pure_check.py
  (non-polar and associating rows, mu = 0): mp.findroot on (p_rho, p_rhorho) with mp.diff.  Exact for those rows; the
  gradient d(T_c, p_c, rho_c)/d(parameters) follows from the same implicit-function formula with mp.diff in the parameters.

* ``oracle_scan`` -- every class, built only on oracle.pure_derivatives (a, p, dp/drho): g(T) = min_rho dp/drho changes
  sign at T_c; bisection in T around a bracketed minimiser (coarse grid in the packing-fraction window ETA_LO .. ETA_HI,
  then golden section).  No second or third density derivative is used, so it is independent of the kernels' formulation.
  The window excludes the liquid-like densities at which strongly polar parameter sets have a second loop.

Measured resolution of the scan against mpmath (python tests/tools/critical_referee.py 200: 200 mu = 0 rows of
pure_batch(seed 2026), sample seed 11), maximum of |scan / mpmath - 1|:
    T_c    1.1e-15
    p_c    1.1e-14
    rho_c  6.1e-8   (the minimiser of a parabola whose values carry fp64 rounding: ~sqrt(eps); 8.5e-8 against the
                     kernel's solver on 2,000 rows of all classes)
The scan's T_c and p_c hold 1e-11 (SCAN_TC_RESOLUTION, SCAN_PC_RESOLUTION: the bound tests/test_critical_referee.py
asserts), so the kernels are compared with the scan at the project's 1e-10 on every class.  rho_c is compared with the scan
at SCAN_RHO_RESOLUTION = 6e-7, ten times the measured maximum (the factor covers other samples), never tighter.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KB = 1.380649e-23
P_UNIT = KB / 1e-30
RHO_UNIT = 1e3 * 6.02214076e23 * 1e-30

ETA_LO, ETA_HI = 0.02, 0.32
N_GRID = 61

# see the module docstring
SCAN_TC_RESOLUTION = 1e-11
SCAN_PC_RESOLUTION = 1e-11
SCAN_RHO_RESOLUTION = 6e-7


def packing_per_density(params, T):
    """eta / rho = pi/6 m d^3, d = sigma (1 - 0.12 exp(-3 eps / T))."""
    d = params[:, 1] * (1.0 - 0.12 * np.exp(-3.0 * params[:, 2] / T))
    return np.pi / 6.0 * params[:, 0] * d**3


def fit_temperature(params):
    """The non-polar fit T_c ~ 1.28 eps m^0.45 (synthetic.pure_batch): only a scale for the scan's first bracket."""
    return 1.28 * params[:, 2] * params[:, 0] ** 0.45


def _dp(orc, params, T, rho):
    return orc.pure_derivatives(params, T, rho)[2]


def min_dp(orc, params, T, golden_iters=46):
    """min over the packing-fraction window of dp/drho at temperature T [n] -> (value [n], minimiser rho [n])."""
    n = len(T)
    ce = packing_per_density(params, T)
    eta = np.linspace(ETA_LO, ETA_HI, N_GRID)
    rho = eta[None, :] / ce[:, None]
    dp = _dp(orc, np.repeat(params, N_GRID, axis=0), np.repeat(T, N_GRID), rho.ravel()).reshape(n, N_GRID)
    k = np.clip(np.argmin(dp, axis=1), 1, N_GRID - 2)
    r = np.arange(n)
    a, b = rho[r, k - 1], rho[r, k + 1]
    gr = 0.5 * (np.sqrt(5.0) - 1.0)
    c, d = b - gr * (b - a), a + gr * (b - a)
    fc, fd = _dp(orc, params, T, c), _dp(orc, params, T, d)
    for _ in range(golden_iters):
        left = fc < fd
        b = np.where(left, d, b)
        a = np.where(left, a, c)
        c_new = np.where(left, b - gr * (b - a), d)
        d_new = np.where(left, c, a + gr * (b - a))
        f_new = _dp(orc, params, T, np.where(left, c_new, d_new))
        fc, fd = np.where(left, f_new, fd), np.where(left, fc, f_new)
        c, d = c_new, d_new
    x = 0.5 * (a + b)
    return _dp(orc, params, T, x), x


def oracle_scan(orc, params, bisections=60):
    """-> T_c [K], p_c [Pa], rho_c [kmol/m3], rho_c [A^-3] of every row by the sign change of min_rho dp/drho."""
    params = np.ascontiguousarray(params, dtype=np.float64)
    n = len(params)
    T0 = fit_temperature(params)
    lo, hi = 0.8 * T0, 1.0 * T0
    for _ in range(40):  # below: a mechanically unstable state exists; above: none in the window
        g, _ = min_dp(orc, params, lo, golden_iters=8)
        bad = g >= 0.0
        if not bad.any():
            break
        lo = np.where(bad, 0.85 * lo, lo)
    assert not bad.any(), "no sub-critical temperature found"
    for _ in range(40):
        g, _ = min_dp(orc, params, hi, golden_iters=8)
        bad = g <= 0.0
        if not bad.any():
            break
        lo = np.where(bad, hi, lo)
        hi = np.where(bad, 1.15 * hi, hi)
    assert not bad.any(), "no super-critical temperature found"
    for _ in range(bisections):
        mid = 0.5 * (lo + hi)
        g, _ = min_dp(orc, params, mid)
        neg = g < 0.0
        lo = np.where(neg, mid, lo)
        hi = np.where(neg, hi, mid)
    Tc = 0.5 * (lo + hi)
    _, rho = min_dp(orc, params, Tc, golden_iters=60)
    _, p, _ = orc.pure_derivatives(params, Tc, rho)
    assert n == len(Tc)
    return Tc, p * Tc * P_UNIT, rho / RHO_UNIT, rho


# ---- mpmath ----------------------------------------------------------------------------------------------------------
AD = [[0.30435038064, 0.95346405973, -1.16100802773], [-0.13585877707, -1.83963831920, 4.52586067320],
      [1.44933285154, 2.01311801180, 0.97512223853], [0.35569769252, -7.37249576667, -12.2810377713],
      [-2.06533084541, 8.23741345333, 5.93975747420]]
BD = [[0.21879385627, -0.58731641193, 3.48695755800], [-1.18964307357, 1.24891317047, -14.9159739347],
      [1.16268885692, -0.50852797392, 15.3720218600]]
CD = [[-0.06467735252, -0.95208758351, -0.62609792333], [0.19758818347, 2.99242575222, 1.29246858189],
      [-0.80875619458, -2.38026356489, 1.65427830900], [0.69028490492, -0.27012609786, -3.43967436378]]


_MP = None


def _mp():
    """mpmath at 50 digits, set ONCE (mp.diff / mp.findroot raise the working precision while they run)."""
    global _MP
    if _MP is None:
        import mpmath as mp

        mp.mp.dps = 50
        _MP = mp
    return _MP


def helmholtz_mp(par, T, rho):
    """50-digit a(T, rho) for ALL four classes, parameters as mpf (so that mp.diff can perturb them): the hard-sphere,
    chain, dispersion and association terms are those of tests/tools/mp_pure_check.py::helmholtz (which takes float
    parameters and mu = 0 only; tests/test_critical_referee.py checks that the two agree to 40 digits there), plus the
    dipole term of Gross & Vrabec (2006) as the model states it: a_dd = phi2^2 / (phi2 - phi3)."""
    mp = _mp()
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import mp_pure_check as chk

    m, sigma, eps, mu, kap, eab, na, nb = par
    T, rho = mp.mpf(T), mp.mpf(rho)
    d = sigma * (1 - mp.mpf("0.12") * mp.exp(-3 * eps / T))
    eta = mp.pi / 6 * m * rho * d**3
    em1 = 1 / (1 - eta)
    hs = m * rho * (4 * eta - 3 * eta**2) * em1**2
    hc = -rho * (m - 1) * mp.log((1 - eta / 2) * em1**3)
    m1, m2 = (m - 1) / m, (m - 1) / m * (m - 2) / m
    I1 = sum((m2 * mp.mpf(chk.A2[i]) + m1 * mp.mpf(chk.A1[i]) + mp.mpf(chk.A0[i])) * eta**i for i in range(7))
    I2 = sum((m2 * mp.mpf(chk.B2[i]) + m1 * mp.mpf(chk.B1[i]) + mp.mpf(chk.B0[i])) * eta**i for i in range(7))
    C1 = 1 / (1 + m * (8 * eta - 2 * eta**2) * em1**4 + (1 - m) * (20 * eta - 27 * eta**2 + 12 * eta**3 - 2 * eta**4) / ((1 - eta) * (2 - eta)) ** 2)
    a = hs + hc - mp.pi * rho**2 * m**2 * (eps / T) * sigma**3 * (2 * I1 + C1 * I2 * m * eps / T)
    if mu != 0:
        s3 = sigma**3
        mu2t = mu * mu / (m * T) * (mp.mpf("1e-19") / mp.mpf(KB))
        if m > 2:
            c = (mp.mpf(1), mp.mpf("0.5"), mp.mpf(0))
        else:
            c = (mp.mpf(1), (m - 1) / m, (m - 1) / m * (m - 2) / m)
        dot = lambda row: sum(mp.mpf(row[j]) * c[j] for j in range(3))
        J1 = sum((dot(AD[i]) + (dot(BD[i]) * eps / T if i < 3 else 0)) * eta**i for i in range(5))
        J2 = sum(dot(CD[i]) * eta**i for i in range(4))
        phi2 = -mp.pi * rho**2 / s3 * J1 * mu2t**2
        phi3 = -mp.mpf(4) / 3 * mp.pi**2 * rho**3 / s3 * J2 * mu2t**3
        a += phi2 * phi2 / (phi2 - phi3)
    if (na + nb) != 0 and kap != 0:
        da = (mp.exp(eab / T) - 1) * sigma**3 * kap
        k = eta * em1
        delta = (1 + k * (mp.mpf("1.5") + mp.mpf("0.5") * k)) * em1 * da
        rhoa, rhob = na * rho, nb * rho
        aux = 1 + (rhoa - rhob) * delta
        sq = mp.sqrt(aux * aux + 4 * rhob * delta)
        xa = 2 / (sq + 1 + (rhob - rhoa) * delta)
        xb = 2 / (sq + 1 - (rhob - rhoa) * delta)
        a += rhoa * (mp.log(xa) - xa / 2 + mp.mpf("0.5")) + rhob * (mp.log(xb) - xb / 2 + mp.mpf("0.5"))
    return a


def _mp_F(mp, helmholtz, par):
    def a_n(T, rho, k):
        return mp.diff(lambda r: helmholtz(par, T, r), rho, k)

    def F(T, rho):
        a2, a3 = a_n(T, rho, 2), a_n(T, rho, 3)
        return 1 + rho * a2, a2 + rho * a3

    return F, a_n


def mp_critical(par, T0, rho0):
    """Exact critical point of one row (any class) from the start (T0 [K], rho0 [A^-3]) -> (T_c, p_c [Pa], rho_c [A^-3],
    p_rhorhorho / kT) as mpf."""
    mp, helmholtz = _mp(), helmholtz_mp
    par = [mp.mpf(float(x)) for x in par]
    F, a_n = _mp_F(mp, helmholtz, par)
    T, rho = mp.findroot(lambda T, r: F(T, r), (mp.mpf(float(T0)), mp.mpf(float(rho0))), tol=mp.mpf(10) ** -35, maxsteps=60)
    a0, a1 = helmholtz(par, T, rho), a_n(T, rho, 1)
    p = (rho - a0 + rho * a1) * T * mp.mpf(KB) / mp.mpf("1e-30")
    p3 = 2 * a_n(T, rho, 3) + rho * a_n(T, rho, 4)
    return T, p, rho, p3


def mp_gradient(par, Tc, rhoc):
    """Exact d(T_c [K], p_c [Pa], rho_c [kmol/m3]) / d(8 parameters) at the mpmath critical point -> float array [3, 8].
    Implicit-function theorem on F = (p_rho, p_rhorho): d(T, rho)/dtheta = -J^-1 dF/dtheta, dp_c/dtheta = p_theta + p_T dT_c
    (p_rho = 0).  The site counts na, nb are differentiated as the continuous variables they are in the model."""
    mp, helmholtz = _mp(), helmholtz_mp
    par = [mp.mpf(float(x)) for x in par]
    unit = mp.mpf(KB) / mp.mpf("1e-30")

    def Fvec(theta, T, rho):
        f, _ = _mp_F(mp, helmholtz, theta)
        return f(T, rho)

    def pres(theta, T, rho):
        a = lambda r: helmholtz(theta, T, r)
        return (rho - a(rho) + rho * mp.diff(a, rho)) * T * unit

    J = mp.matrix(2, 2)
    for j, var in enumerate(("T", "rho")):
        for i in range(2):
            if var == "T":
                J[i, j] = mp.diff(lambda t: Fvec(par, t, rhoc)[i], Tc)
            else:
                J[i, j] = mp.diff(lambda r: Fvec(par, Tc, r)[i], rhoc)
    pT = mp.diff(lambda t: pres(par, t, rhoc), Tc)
    det = J[0, 0] * J[1, 1] - J[0, 1] * J[1, 0]
    out = np.zeros((3, 8))
    for k in range(8):
        if k == 3 and par[3] == 0:
            continue  # mu = 0: the Helmholtz energy is even in mu, the derivative vanishes
        if k in (4, 5, 6, 7) and (par[6] + par[7] == 0 or par[4] == 0):
            # no association term in this row; the kernels differentiate the value they evaluate, which has none either
            # (kappa_ab = 0 with sites present is not a row of pure_batch)
            continue

        def with_k(x):
            th = list(par)
            th[k] = x
            return th

        dF = mp.matrix([mp.diff(lambda x: Fvec(with_k(x), Tc, rhoc)[i], par[k]) for i in range(2)])
        d = [-(J[1, 1] * dF[0] - J[0, 1] * dF[1]) / det, -(J[0, 0] * dF[1] - J[1, 0] * dF[0]) / det]
        pth = mp.diff(lambda x: pres(with_k(x), Tc, rhoc), par[k])
        out[0, k] = float(d[0])
        out[1, k] = float(pth + pT * d[0])
        out[2, k] = float(d[1] / mp.mpf(RHO_UNIT))
    return out


MP_SEED = 11    # mu = 0 rows compared with mpmath
SCAN_SEED = 13  # rows of all classes compared with the oracle scan
VLE_SEED = 7    # rows on which the consistency with the VLE solve is checked (CPU: the oracle alone solves them all)
F_SUB = 0.90    # sub-critical temperature of that check, as a fraction of T_c
DP_ROUND = 8 * 2.220446049250313e-16  # rounding of dp/drho = 1 + rho a'' (terms of order one) in double precision


def vle_sample():
    return sample(400, seed=VLE_SEED)


def dp_noise(orc, params, T, rho, ulps=8):
    """Rounding of the oracle's dp/drho in double precision at (T, rho), from the oracle alone: dp/drho = 1 + rho a'' is a
    difference of numbers of order one (DP_ROUND), and a'' itself carries the rounding of the association / dipole terms.
    That part is sampled: over +-`ulps` ulps of rho and of T the exact value moves by < 1e-15 |d(dp/drho)/d ln x| -- nothing
    next to the evaluation's rounding, whose spread (max - min over the 4 ulps + 1 samples) is therefore visible directly.
    Bound: DP_ROUND + 2 spreads (a further sample lies outside the observed range of 33 with probability 2/34)."""
    vals = [orc.pure_derivatives(params, T, rho)[2]]
    for k in range(1, ulps + 1):
        for sgn in (-np.inf, np.inf):
            r, t = rho.copy(), T.copy()
            for _ in range(k):
                r, t = np.nextafter(r, sgn), np.nextafter(t, sgn)
            vals.append(orc.pure_derivatives(params, T, r)[2])
            vals.append(orc.pure_derivatives(params, t, rho)[2])
    vals = np.stack(vals)
    return DP_ROUND + 2.0 * (vals.max(axis=0) - vals.min(axis=0))


def scan_central_differences(orc, params, rel=1e-4):
    """d(T_c, p_c, rho_c)/d(parameter k) by central differences of the oracle scan -> [n, 3, 8] (zero columns where the
    parameter is zero: a row's class is not changed)."""
    n = len(params)
    out = np.zeros((n, 3, 8))
    for k in range(8):
        h = rel * np.abs(params[:, k])
        if not h.any():
            continue
        hp, hm = params.copy(), params.copy()
        hp[:, k] += h
        hm[:, k] -= h
        a, b = oracle_scan(orc, hp), oracle_scan(orc, hm)
        with np.errstate(invalid="ignore", divide="ignore"):
            for o in range(3):
                out[:, o, k] = np.where(h > 0, (a[o] - b[o]) / (2 * h), 0.0)
    return out


def sample(n, seed, mu_zero=None, pool=200_000):
    """Seeded subset of pure_batch parameter rows, all four classes; mu_zero=True: non-polar + associating only."""
    from feos_torch_amd.synthetic import pure_batch

    P, _ = pure_batch(pool, seed=2026)
    if mu_zero is True:
        P = P[P[:, 3] == 0.0]
    elif mu_zero is False:
        P = P[P[:, 3] != 0.0]
    idx = np.random.default_rng(seed).choice(len(P), size=n, replace=False)
    return np.ascontiguousarray(P[np.sort(idx)])


if __name__ == "__main__":
    from oracle import pyoracle as orc

    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    P = sample(n, seed=11, mu_zero=True)
    Tc, pc, rc, rr = oracle_scan(orc, P)
    e = np.zeros((n, 3))
    for i in range(n):
        T, p, rho, p3 = mp_critical(P[i], Tc[i], rr[i])
        e[i] = [abs(Tc[i] / float(T) - 1), abs(pc[i] / float(p) - 1), abs(rr[i] / float(rho) - 1)]
    print("scan vs mpmath, max rel: T_c %.3e  p_c %.3e  rho_c %.3e" % tuple(e.max(axis=0)))
