"""Referee and input set for PcSaftMix.liquid_density / vapor_density (test infrastructure, numpy only).

Root.  With p(rho), dp/drho the reduced pressure and its slope along the composition line rho_i = x_i rho, eta = packing rho
and p_spec = p [Pa] 1e-30 / (k_B T), the roots are defined as in include/pcsaft_hip.h (pcs_mix_density):
  liquid, rho_s = 0.5 / packing:
    p(rho_s) >= p_spec: the largest rho <= rho_s with p = p_spec, provided dp/drho > 0 on all of [rho, rho_s] (else the liquid
                        branch ends above p_spec: status ENDS);
    p(rho_s) <  p_spec: the smallest rho > rho_s with p = p_spec, dp/drho > 0 and eta < 0.74 (else status NONE);
  vapour: the smallest rho > 0 with p = p_spec, provided dp/drho > 0 on (0, rho] (else ENDS).
They are found here without any of the kernel's code or decisions: p from oracle.mix_derivatives_exact and the slope
x_0 col19 + x_1 col20 of oracle.mix_derivatives_vjp_exact(gp = 1) are scanned on the FIXED grid eta = 0, D_ETA, 2 D_ETA, ...
away from the start of the branch; the first cell in which the pressure passes p_spec or the slope turns non-positive holds
the event.  Where the slope turned, the spinodal inside the cell is located by bisection on the slope's sign and its pressure
decides between a root before it and ENDS.  The root is then taken inside its bracket by Newton / bisection in long double to
|d rho| <= 1e-16 rho.

Gradient.  Implicit-function theorem on p_model(theta, T, rho x) = p [Pa] 1e-30 / (k_B T), from ONE
mix_derivatives_vjp_exact(gp = 1) call G [n,21] at the root, s = x_0 G19 + x_1 G20:
    d rho / d(parameters, kij) = -G[:, :18] / s        d rho / dT = -(G18 + p_spec / T) / s
    d rho / dp [Pa] = 1e-30 / (k_B T s)                d rho / dx = -rho (G19 - G20) / s
prec=1 (long double) is the referee, prec=0 (the same code in double) the yardstick of what fp64 delivers.

Input set (per phase; the GPU test uses the same): the rows of tests/tools/mix_temperature_referee.py -- the 192 parameter
rows of synthetic.mix_batch(192, 2024), 6 association classes x 32, at T = s T_batch for s in (0.85, 1.0, 1.2) -- at the
pressures FACTORS[phase] x the oracle's bubble (liquid) / dew (vapour) pressure at (T, x); rows whose bubble / dew point the
oracle does not solve stay in the batch at 1e5 Pa as wave mates and are not compared.  The liquid set has two further
blocks, the same rows at x = 0 and at x = 1, at 3 x the bubble pressure of the x = 0.5 mixture.  A row is kept when the
referee finds the root and the reduced dp/drho there is >= MIN_SLOPE: nearer the spinodal the root is ill-conditioned in p
and measures nothing.  At most CAP of the rows of any (class, factor, pressure) cell of a phase may be dropped
(tests/test_mix_density_referee.py).
"""
import numpy as np

import mix_temperature_referee as tref

LIQUID, VAPOUR = 0, 1
FACTORS = {LIQUID: (1.0, 3.0, 30.0), VAPOUR: (1.0, 0.5, 0.05)}
PURE_FACTOR = 3.0  # pure-limit blocks: x the bubble pressure of the x = 0.5 mixture
MIN_SLOPE = 0.05
CAP = 0.10
D_ETA = 0.005
ETA_START, ETA_MAX = 0.5, 0.74
KB = 1.380649e-23
P_RED = 1e-30 / KB  # p_spec = p [Pa] P_RED / T
OK, ENDS, NONE, INVALID = 0, 1, 2, 3  # referee status


def packing(P, T, x):
    """zeta_3 / rho along the line: pi/6 sum_i x_i m_i d_i^3, d_i = sigma_i (1 - 0.12 exp(-3 eps_i / T))"""
    P = P.reshape(len(T), 2, 8)
    d = P[:, :, 1] * (1.0 - 0.12 * np.exp(-3.0 * P[:, :, 2] / T[:, None]))
    xx = np.stack((x, 1.0 - x), axis=1)
    return np.pi / 6.0 * (xx * P[:, :, 0] * d ** 3).sum(axis=1)


def line(orc, P, K, T, x, rho, prec=1):
    """p [n], dp/drho [n] along the line at the total densities rho, and the full G [n,21] of gp = 1"""
    n = len(T)
    r2 = np.stack((x * rho, (1.0 - x) * rho), axis=1)
    z, z2 = np.zeros(n), np.zeros((n, 2))
    G = orc.mix_derivatives_vjp_exact(P, K, T, r2, z, np.ones(n), z2, z2, prec=prec)
    p = orc.mix_derivatives_exact(P, K, T, r2)[1] if prec else orc.mix_derivatives(P, K, T, r2, robust=True)[1]
    return p, x * G[:, 19] + (1.0 - x) * G[:, 20], G


def _bisect_slope(orc, P, K, T, x, lo, hi, positive_at_lo, iters=48):
    """the density in (lo, hi) where dp/drho changes sign; positive_at_lo: dp(lo) > 0 >= dp(hi), else the other way round"""
    lo, hi = lo.copy(), hi.copy()
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        _, s, _ = line(orc, P, K, T, x, mid)
        same = (s > 0) == positive_at_lo
        lo, hi = np.where(same, mid, lo), np.where(same, hi, mid)
    return 0.5 * (lo + hi)


def _polish(orc, P, K, T, x, p_spec, lo, hi, max_it=200):
    """root of p = p_spec in [lo, hi], p(lo) < p_spec <= p(hi): Newton inside the bracket, else bisection"""
    n = len(T)
    rising = np.ones(n, dtype=bool)
    rho = 0.5 * (lo + hi)
    lo, hi = lo.copy(), hi.copy()
    done = np.zeros(n, dtype=bool)
    for _ in range(max_it):
        idx = np.nonzero(~done)[0]
        if len(idx) == 0:
            break
        p, s, _ = line(orc, P[idx], K[idx], T[idx], x[idx], rho[idx])
        f = p - p_spec[idx]
        below = (f < 0) == rising[idx]  # on lo's side of the root
        lo[idx] = np.where(below, rho[idx], lo[idx])
        hi[idx] = np.where(below, hi[idx], rho[idx])
        with np.errstate(invalid="ignore", divide="ignore"):
            new = rho[idx] - f / s
        inside = np.isfinite(new) & (new >= lo[idx]) & (new <= hi[idx]) & (new > 0) & (s > 0)  # rho = 0 itself is never evaluated
        new = np.where(inside, new, 0.5 * (lo[idx] + hi[idx]))
        conv = (np.abs(new - rho[idx]) <= 1e-16 * rho[idx]) | (f == 0) | (hi[idx] - lo[idx] <= 4.5e-16 * hi[idx])  # or the bracket is two neighbouring doubles
        rho[idx] = new
        done[idx[conv]] = True
    return np.where(done, rho, np.nan)


def solve(orc, P, K, T, p_pa, x, phase):
    """-> rho [n] (NaN unless status OK), dpdrho [n], status [n].  Vectorised over the rows."""
    n = len(T)
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(n, 2, 8)
    status = np.full(n, INVALID)
    rho_out, slope_out = np.full(n, np.nan), np.full(n, np.nan)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(T) & np.isfinite(p_pa) & np.isfinite(x) & (T > 0) & (p_pa > 0) & (x >= 0) & (x <= 1)
    v = np.nonzero(valid)[0]
    if len(v) == 0:
        return rho_out, slope_out, status
    Pv, Kv, Tv, xv = P[v], K[v], T[v], x[v]
    ps = p_pa[v] * P_RED / Tv
    pk = packing(Pv, Tv, xv)
    m = len(v)
    # the grid walk: direction and grid per row
    if phase == LIQUID:
        p_s, _, _ = line(orc, Pv, Kv, Tv, xv, ETA_START / pk)
        up = p_s < ps
        eta0 = np.full(m, ETA_START)
    else:
        up = np.ones(m, dtype=bool)
        eta0 = np.zeros(m)
    strict = ~up if phase == LIQUID else np.ones(m, dtype=bool)
    st = np.full(m, -1)
    lo, hi = np.full(m, np.nan), np.full(m, np.nan)  # bracket of the root in density, lo < hi
    turned = np.zeros(m, dtype=bool)                  # the event of the cell was the slope turning non-positive
    prev = eta0 / pk
    if phase == LIQUID:
        _, s0, _ = line(orc, Pv, Kv, Tv, xv, prev)
        st[strict & ~(s0 > 0)] = ENDS  # no liquid branch at eta = 0.5
    k = 0
    while (st == -1).any():
        k += 1
        live = np.nonzero(st == -1)[0]
        eta = eta0[live] + np.where(up[live], 1.0, -1.0) * k * D_ETA
        top = up[live] & (eta > ETA_MAX + 1e-12) if phase == LIQUID else eta > 0.9
        out = top | (eta <= 0)
        st[live[out]] = NONE if phase == LIQUID else ENDS
        live, eta = live[~out], eta[~out]
        if len(live) == 0:
            continue
        eta = np.minimum(eta, ETA_MAX) if phase == LIQUID else eta
        cur = eta / pk[live]
        p, s, _ = line(orc, Pv[live], Kv[live], Tv[live], xv[live], cur)
        f = p - ps[live]
        crossed = np.where(up[live], f >= 0, f <= 0)
        bad_slope = strict[live] & ~(s > 0)
        event = crossed | bad_slope | ~np.isfinite(p)
        e = live[event]
        lo[e] = np.minimum(prev[e], cur[event])
        hi[e] = np.maximum(prev[e], cur[event])
        turned[e] = (bad_slope & ~crossed)[event]
        st[e] = np.where(np.isfinite(p[event]), -2, NONE)
        prev[live] = cur
    # cells whose slope turned before the pressure passed p_spec: the spinodal inside decides
    t = np.nonzero((st == -2) & turned)[0]
    if len(t):
        spin = _bisect_slope(orc, Pv[t], Kv[t], Tv[t], xv[t], lo[t], hi[t], up[t])
        p_end, _, _ = line(orc, Pv[t], Kv[t], Tv[t], xv[t], spin)
        reaches = np.where(up[t], p_end >= ps[t], p_end <= ps[t])
        st[t[~reaches]] = ENDS
        lo[t] = np.where(up[t], lo[t], spin)
        hi[t] = np.where(up[t], spin, hi[t])
    # cells the pressure passed with the slope non-positive at the far end: a spinodal lies between root and far end (vapour /
    # liquid from above), the bracket still holds exactly one sign change of p - p_spec on the branch side
    r = np.nonzero(st == -2)[0]
    if len(r):
        root = _polish(orc, Pv[r], Kv[r], Tv[r], xv[r], ps[r], lo[r], hi[r])
        safe = np.where(np.isfinite(root), root, lo[r])
        _, s, _ = line(orc, Pv[r], Kv[r], Tv[r], xv[r], safe)
        good = np.isfinite(root) & (s > 0) & (root * pk[r] < ETA_MAX)
        st[r] = np.where(good, OK, NONE if phase == LIQUID else ENDS)
        rho_out[v[r]] = np.where(good, root, np.nan)
        slope_out[v[r]] = np.where(good, s, np.nan)
    status[v] = st
    return rho_out, slope_out, status


def gradient(orc, P, K, T, p_pa, x, rho, prec=1):
    """[n,21]: d rho [A^-3] / d(16 parameters, kij0, kij1, T, p [Pa], x) at the root rho"""
    _, s, G = line(orc, P, K, T, x, rho, prec=prec)
    ps = p_pa * P_RED / T
    out = np.empty((len(T), 21))
    out[:, :18] = -G[:, :18] / s[:, None]
    out[:, 18] = -(G[:, 18] + ps / T) / s
    out[:, 19] = P_RED / (T * s)
    out[:, 20] = -rho * (G[:, 19] - G[:, 20]) / s
    return out


class Inputs:
    pass


_CACHE = {}


def inputs(orc, phase):
    """The input set of one phase, block-major (pressure factor, then temperature factor, then parameter row).  Cached per process."""
    if phase in _CACHE:
        return _CACHE[phase]
    b = tref.inputs(orc, bool(phase))
    solved = np.isfinite(b.rho4).all(axis=1)
    blocks = [(b.z, np.where(solved, f * b.p_spec, 1e5), solved) for f in FACTORS[phase]]
    if phase == LIQUID:
        half = np.full(b.n, 0.5)
        p_half, _, st = orc.mix_bubble_dew(b.P, b.K, b.T, half, b.p_spec, False, prec=1)
        ok_half = ~st & np.isfinite(p_half) & (p_half > 0)
        p_pure = np.where(ok_half, PURE_FACTOR * np.where(ok_half, p_half, 1.0), 1e5)
        blocks += [(np.zeros(b.n), p_pure, ok_half), (np.ones(b.n), p_pure, ok_half)]
    c = Inputs()
    nb = len(blocks)
    c.phase, c.nblocks, c.n = phase, nb, nb * b.n
    c.P, c.K, c.T = np.tile(b.P, (nb, 1, 1)), np.tile(b.K, (nb, 1)), np.tile(b.T, nb)
    c.x = np.concatenate([blk[0] for blk in blocks])
    c.p = np.concatenate([blk[1] for blk in blocks])
    c.compared = np.concatenate([blk[2] for blk in blocks])
    c.block = np.repeat(np.arange(nb), b.n)
    c.cls, c.factor = np.tile(b.cls, nb), np.tile(b.factor, nb)
    c.cell = (c.block * len(tref.FACTORS) + c.factor) * tref.N_CLASSES + c.cls
    c.base_rho4 = np.tile(b.rho4, (nb, 1))
    c.rho, c.dpdrho, c.status = solve(orc, c.P, c.K, c.T, c.p, c.x, phase)
    with np.errstate(invalid="ignore"):
        c.keep = c.compared & (c.status == OK) & (c.dpdrho >= MIN_SLOPE)
    c.dropped_share = np.array([np.mean(~c.keep[c.cell == k]) for k in range(c.cell.max() + 1)])
    kk = np.nonzero(c.keep)[0]
    c.grad, c.grad64 = np.full((c.n, 21), np.nan), np.full((c.n, 21), np.nan)
    for prec, dst in ((1, c.grad), (0, c.grad64)) if len(kk) else ():
        dst[kk] = gradient(orc, c.P[kk], c.K[kk], c.T[kk], c.p[kk], c.x[kk], c.rho[kk], prec=prec)
    _CACHE[phase] = c
    return c


def interleave(n, nblocks):
    """a fixed permutation that mixes the pressure and temperature blocks within a wave: position -> row"""
    return np.arange(n).reshape(nblocks * len(tref.FACTORS), -1).T.ravel()
