"""Referee and input set for GcPcSaftMix.liquid_density / vapor_density (test infrastructure, numpy + oracle only): the gc twin
of tests/tools/mix_density_referee.py.  It takes none of the kernel's decisions.

Root.  With p(rho), dp/drho the reduced pressure and its slope along the composition line rho_i = x_i rho, eta = packing rho
and p_spec = p [Pa] 1e-30 / (k_B T), the roots are defined as in include/pcsaft_hip.h (pcs_mix_density / pcs_gc_density):
  liquid, rho_s = 0.5 / packing:
    p(rho_s) >= p_spec: the largest rho <= rho_s with p = p_spec, provided dp/drho > 0 on all of [rho, rho_s] (else the liquid
                        branch ends above p_spec: status ENDS);
    p(rho_s) <  p_spec: the smallest rho > rho_s with p = p_spec, dp/drho > 0 and eta < 0.74 (else status NONE);
  vapour: the smallest rho > 0 with p = p_spec, provided dp/drho > 0 on (0, rho] (else ENDS).
p is oracle.gc_derivatives(prec=1): long double, rounded to double on return.  The packing fraction is restated here from the
dense encoding, pi/6 sum_i x_i sum_seg count m d^3 with d = sigma (1 - 0.12 exp(-3 epsilon_k / T)).  The branch is scanned on
the FIXED grid eta = start, start +- D_ETA, ... away from its start; on the grid and inside a cell the SIGN of the slope comes
from a central difference of that p (relative step FD_STEP; p carries 1e-16 of rounding, so the difference resolves slopes down
to ~1e-9 of p / rho: rows that close to a spinodal are dropped by MIN_SLOPE anyway).  The first cell in which the pressure
passes p_spec or the slope turns non-positive holds the event; where the slope turned, the spinodal inside the cell is
located by bisection on the slope's sign and its pressure decides between a root before it and ENDS.  The root is then taken
inside its bracket by Newton / bisection to |d rho| <= 1e-16 rho.

Slope and gradient at the root: oracle.gc_derivatives_vjp_exact.  A first call with gp = 1 gives per row
dp/d(phi_0, phi_1, T, rho_0, rho_1) and with it s = x_0 g_rho0 + x_1 g_rho1 = dp/drho along the line.  For an upstream
gradient w of rho, a second call with gp = -w / s gives the weighted sums for k_ab and the segment table and the per-row phi
columns; T, p and x follow the formulas of mix_density_referee.gradient:
    d rho / dT = -(g_T + p_spec / T) / s        d rho / dp [Pa] = 1e-30 / (k_B T s)        d rho / dx = -rho (g_rho0 - g_rho1) / s.
The referee's table entries are Richardson differences (oracle/pyoracle.py), and it offers no fp64 twin.

Pure limits.  At x = 0 and x = 1 the oracle is evaluated at the partial densities (0, rho) / (rho, 0) themselves: its pressure,
its duals and its table differences are finite there (tests/test_gc_density_referee.py asserts it on the kept rows).

Input set (per phase; the GPU test uses the same): the rows of gc_temperature_referee.inputs(oracle, dew) -- 3 x 384 gc rows,
every model class the molecule library has, at T = 0.85 / 1.0 / 1.2 T_batch -- at the pressures FACTORS[phase] x the oracle's
bubble (liquid) / dew (vapour) pressure at (T, x); rows whose bubble / dew point the oracle does not solve stay in the batch at
1e5 Pa as wave mates and are not compared.  The liquid set has two further blocks, the same rows at x = 0 and at x = 1, at 3 x
the bubble pressure of the x = 0.5 mixture.  A row is kept when the referee finds the root and the reduced dp/drho there is
>= MIN_SLOPE: nearer the spinodal the root is ill-conditioned in p and measures nothing.  At most CAP of the rows of any
(class, temperature factor, pressure block) cell may be dropped (tests/test_gc_density_referee.py).
"""
import numpy as np

import gc_temperature_referee as tref

LIQUID, VAPOUR = 0, 1
FACTORS = {LIQUID: (1.0, 3.0, 30.0), VAPOUR: (1.0, 0.5, 0.05)}
PURE_FACTOR = 3.0  # pure-limit blocks: x the bubble pressure of the x = 0.5 mixture
MIN_SLOPE = 0.05
CAP = 0.10
D_ETA = 0.005
FD_STEP = 1e-6
ETA_START, ETA_MAX = 0.5, 0.74
KB = 1.380649e-23
P_RED = 1e-30 / KB  # p_spec = p [Pa] P_RED / T
OK, ENDS, NONE, INVALID = 0, 1, 2, 3  # referee status
SEED = 2044


class Rows:
    """The model side of a batch: dense encoding and phi; `idx` arguments below pick rows of it."""

    def __init__(self, orc, enc, phi):
        self.orc, self.enc, self.phi = orc, enc, phi

    def sub(self, idx):
        return tref.sub_enc(self.enc, idx), np.ascontiguousarray(self.phi[idx])


def packing(enc, idx, T, x):
    """zeta_3 / rho along the line: pi/6 sum_i x_i sum_seg count m d^3, d = sigma (1 - 0.12 exp(-3 eps / T))"""
    seg = enc["seg"]
    d = seg[None, :, 1] * (1.0 - 0.12 * np.exp(-3.0 * seg[None, :, 2] / T[:, None]))  # [n,S]
    per = (enc["counts"][idx] * (seg[None, None, :, 0] * d[:, None, :] ** 3)).sum(axis=2)  # [n,2]
    return np.pi / 6.0 * (x * per[:, 0] + (1.0 - x) * per[:, 1])


def _r2(x, rho):
    return np.stack((x * rho, (1.0 - x) * rho), axis=1)


def pressure(m, idx, T, x, rho):
    """p [n] (long double, rounded) at the total densities rho"""
    enc, phi = m.sub(idx)
    return m.orc.gc_derivatives(enc, phi, T, _r2(x, rho), prec=1)[1]


def line(m, idx, T, x, rho):
    """p [n] and the central-difference slope [n] (its sign is what the scan uses)"""
    p = pressure(m, idx, T, x, rho)
    s = (pressure(m, idx, T, x, rho * (1.0 + FD_STEP)) - pressure(m, idx, T, x, rho * (1.0 - FD_STEP))) / (2.0 * FD_STEP * rho)
    return p, s


def exact(m, idx, T, x, rho, gp=None):
    """gc_derivatives_vjp_exact with the weight gp on the pressure alone (None: 1) -> grad_row [n,5], grad_seg, grad_kab, s [n]"""
    enc, phi = m.sub(idx)
    n = len(T)
    z, z2 = np.zeros(n), np.zeros((n, 2))
    grow, gseg, gkab = m.orc.gc_derivatives_vjp_exact(enc, phi, T, _r2(x, rho), z, np.ones(n) if gp is None else gp, z2, z2)
    return grow, gseg, gkab, x * grow[:, 3] + (1.0 - x) * grow[:, 4]


def _bisect_slope(m, idx, T, x, lo, hi, positive_at_lo, iters=40):
    """the density in (lo, hi) where dp/drho changes sign; positive_at_lo: dp(lo) > 0 >= dp(hi), else the other way round"""
    lo, hi = lo.copy(), hi.copy()
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        _, s = line(m, idx, T, x, mid)
        same = (s > 0) == positive_at_lo
        lo, hi = np.where(same, mid, lo), np.where(same, hi, mid)
    return 0.5 * (lo + hi)


def _polish(m, idx, T, x, p_spec, lo, hi, max_it=200):
    """root of p = p_spec in [lo, hi], p(lo) < p_spec <= p(hi): Newton inside the bracket, else bisection"""
    n = len(T)
    rho = 0.5 * (lo + hi)
    lo, hi = lo.copy(), hi.copy()
    done = np.zeros(n, dtype=bool)
    for _ in range(max_it):
        k = np.nonzero(~done)[0]
        if len(k) == 0:
            break
        p, s = line(m, idx[k], T[k], x[k], rho[k])
        f = p - p_spec[k]
        below = f < 0
        lo[k] = np.where(below, rho[k], lo[k])
        hi[k] = np.where(below, hi[k], rho[k])
        with np.errstate(invalid="ignore", divide="ignore"):
            new = rho[k] - f / s
        inside = np.isfinite(new) & (new >= lo[k]) & (new <= hi[k]) & (new > 0) & (s > 0)
        new = np.where(inside, new, 0.5 * (lo[k] + hi[k]))
        conv = (np.abs(new - rho[k]) <= 1e-16 * rho[k]) | (f == 0) | (hi[k] - lo[k] <= 4.5e-16 * hi[k])  # or the bracket is two neighbouring doubles
        rho[k] = new
        done[k[conv]] = True
    return np.where(done, rho, np.nan)


def solve(m, idx, T, p_pa, x, phase, exact_slope=True):
    """-> rho [n] (NaN unless status OK), dpdrho [n] (exact, of the first gc_derivatives_vjp_exact call), status [n],
    grad_row [n,5] of that call (NaN unless OK).  Vectorised over the rows; idx: rows of m.  exact_slope=False: status and
    root only, the slope at the root is the central difference and grad_row stays NaN (no table differences are paid)."""
    n = len(T)
    idx = np.asarray(idx)
    status = np.full(n, INVALID)
    rho_out, slope_out, grow_out = np.full(n, np.nan), np.full(n, np.nan), np.full((n, 5), np.nan)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(T) & np.isfinite(p_pa) & np.isfinite(x) & (T > 0) & (p_pa > 0) & (x >= 0) & (x <= 1)
    v = np.nonzero(valid)[0]
    if len(v) == 0:
        return rho_out, slope_out, status, grow_out
    iv, Tv, xv = idx[v], T[v], x[v]
    ps = p_pa[v] * P_RED / Tv
    pk = packing(m.enc, iv, Tv, xv)
    k_rows = len(v)
    if phase == LIQUID:
        p_s, s0 = line(m, iv, Tv, xv, ETA_START / pk)
        up = p_s < ps
        eta0 = np.full(k_rows, ETA_START)
    else:
        up = np.ones(k_rows, dtype=bool)
        eta0 = np.zeros(k_rows)
    strict = ~up if phase == LIQUID else np.ones(k_rows, dtype=bool)
    st = np.full(k_rows, -1)
    lo, hi = np.full(k_rows, np.nan), np.full(k_rows, np.nan)  # bracket of the root in density, lo < hi
    turned = np.zeros(k_rows, dtype=bool)                      # the event of the cell was the slope turning non-positive
    prev = eta0 / pk
    if phase == LIQUID:
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
        p, s = line(m, iv[live], Tv[live], xv[live], cur)
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
        spin = _bisect_slope(m, iv[t], Tv[t], xv[t], lo[t], hi[t], up[t])
        p_end = pressure(m, iv[t], Tv[t], xv[t], spin)
        reaches = np.where(up[t], p_end >= ps[t], p_end <= ps[t])
        st[t[~reaches]] = ENDS
        lo[t] = np.where(up[t], lo[t], spin)
        hi[t] = np.where(up[t], spin, hi[t])
    r = np.nonzero(st == -2)[0]
    if len(r):
        root = _polish(m, iv[r], Tv[r], xv[r], ps[r], lo[r], hi[r])
        safe = np.where(np.isfinite(root), root, lo[r])
        if exact_slope:
            grow, _, _, s = exact(m, iv[r], Tv[r], xv[r], safe)
        else:
            grow, s = np.full((len(r), 5), np.nan), line(m, iv[r], Tv[r], xv[r], safe)[1]
        good = np.isfinite(root) & (s > 0) & (root * pk[r] < ETA_MAX)
        st[r] = np.where(good, OK, NONE if phase == LIQUID else ENDS)
        rho_out[v[r]] = np.where(good, root, np.nan)
        slope_out[v[r]] = np.where(good, s, np.nan)
        grow_out[v[r]] = np.where(good[:, None], grow, np.nan)
    status[v] = st
    return rho_out, slope_out, status, grow_out


def row_gradient(T, p_pa, x, rho, s, grow):
    """[n,5]: d rho [A^-3] / d(phi_0, phi_1, T, p [Pa], x) at the root from the first call's grad_row and s"""
    ps = p_pa * P_RED / T
    out = np.empty((len(T), 5))
    out[:, :2] = -grow[:, :2] / s[:, None]
    out[:, 2] = -(grow[:, 2] + ps / T) / s
    out[:, 3] = P_RED / (T * s)
    out[:, 4] = -rho * (grow[:, 3] - grow[:, 4]) / s
    return out


class Inputs:
    pass


_CACHE = {}


def inputs(orc, phase):
    """The input set of one phase, block-major (pressure block, then temperature factor, then row).  Cached per process."""
    if phase in _CACHE:
        return _CACHE[phase]
    b = tref.inputs(orc, bool(phase))
    solved = np.isfinite(b.rho4).all(axis=1)
    blocks = [(b.z, np.where(solved, f * b.p_spec, 1e5), solved) for f in FACTORS[phase]]
    if phase == LIQUID:
        half = np.full(b.n, 0.5)
        p_half, _, st = orc.gc_bubble_dew(b.enc, b.phi, b.T, half, b.p_spec, False, prec=1)
        ok_half = ~st & np.isfinite(p_half) & (p_half > 0)
        p_pure = np.where(ok_half, PURE_FACTOR * np.where(ok_half, p_half, 1.0), 1e5)
        blocks += [(np.zeros(b.n), p_pure, ok_half), (np.ones(b.n), p_pure, ok_half)]
    c = Inputs()
    nb = len(blocks)
    c.phase, c.nblocks, c.n, c.base = phase, nb, nb * b.n, b
    c.m = Rows(orc, b.enc, b.phi)
    c.row = np.tile(np.arange(b.n), nb)  # row of the base set (encoding, phi, structure lists)
    c.phi, c.T = np.tile(b.phi, (nb, 1)), np.tile(b.T, nb)
    c.x = np.concatenate([blk[0] for blk in blocks])
    c.p = np.concatenate([blk[1] for blk in blocks])
    c.compared = np.concatenate([blk[2] for blk in blocks])
    c.block = np.repeat(np.arange(nb), b.n)
    c.cls, c.factor = np.tile(b.cls, nb), np.tile(b.factor, nb)
    c.classes = np.unique(b.cls)
    c.cell = (c.block * len(tref.FACTORS) + c.factor) * tref.N_KEYS + c.cls
    c.cells = np.unique(c.cell)
    c.base_rho4 = np.tile(b.rho4, (nb, 1))
    c.rho, c.dpdrho, c.status, c.grow = solve(c.m, c.row, c.T, c.p, c.x, phase)
    with np.errstate(invalid="ignore"):
        c.keep = c.compared & (c.status == OK) & (c.dpdrho >= MIN_SLOPE)
    c.dropped_share = {int(k): float(np.mean(~c.keep[c.cell == k])) for k in c.cells}
    c.grad_row = np.full((c.n, 5), np.nan)
    kk = c.keep
    c.grad_row[kk] = row_gradient(c.T[kk], c.p[kk], c.x[kk], c.rho[kk], c.dpdrho[kk], c.grow[kk])
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CACHE[phase] = c
    return c


def weighted(orc, c):
    """The referee of the gradient test, computed once per phase: seeded upstream gradients g ~ U(0.5, 1.5) of rho [A^-3] on the
    kept rows (0 elsewhere) and, per model class (the weights masked to it, gc_point_rows.groups), the second call with
    gp = -g / s: {class: dict(rows (indices), grad_kab [S,S], grad_seg [S,8], phi [m,2] = g d rho / d phi)}, and 'all' as the
    sum over the classes (both sums are linear in the weights)."""
    key = ("weighted", c.phase)
    if key not in _CACHE:
        g = np.where(c.keep, np.random.default_rng(SEED + c.phase).uniform(0.5, 1.5, c.n), 0.0)
        out = {"g": g, "groups": {}}
        S = c.m.enc["S"]
        tot = {"grad_kab": np.zeros((S, S)), "grad_seg": np.zeros((S, 8))}
        for k in c.classes:
            rows = np.nonzero(c.keep & (c.cls == k))[0]
            if len(rows) == 0:
                continue
            grow, gseg, gkab, _ = exact(c.m, c.row[rows], c.T[rows], c.x[rows], c.rho[rows], gp=-g[rows] / c.dpdrho[rows])
            out["groups"][int(k)] = {"rows": rows, "grad_kab": gkab, "grad_seg": gseg, "phi": grow[:, :2]}
            tot["grad_kab"] += gkab
            tot["grad_seg"] += gseg
        out["all"] = tot
        _CACHE[key] = out
    return _CACHE[key]


def interleave(n, nblocks):
    """a fixed permutation that mixes the pressure and temperature blocks within a wave: position -> row"""
    return np.arange(n).reshape(nblocks * len(tref.FACTORS), -1).T.ravel()
