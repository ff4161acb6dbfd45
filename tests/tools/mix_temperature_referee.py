"""Referee and input set for PcSaftMix.bubble_temperature / dew_temperature (test infrastructure, numpy only).

Referee: the T with p_oracle(T, z) = p_spec by a bracketed secant / bisection on f = ln p - ln p_spec in x = 1/T, over
oracle.pyoracle.mix_bubble_dew in its most precise mode (prec=1: long double, 1e-17 step tolerance), every evaluation started
from the previous pressure.  Its gradient is the implicit-function quotient of the oracle's exact pressure gradient at the
solved state: dT/dtheta = -g[:, :18] / g[:, 18], dT/dp_spec = 1 / g[:, 18]  (g = mix_bubble_dew_grad(..., exact=True)).

Input set (the GPU test uses the same): the parameter rows of synthetic.mix_batch(N_ROWS, SEED) -- 6 association classes x 32
rows -- at T_grid = s T_batch for the factors FACTORS (T_batch is 0.6 of the lower critical-temperature estimate, so all stay
sub-critical), both problems, p_spec = the oracle's pressure at T_grid: the exact answer is T_grid.  A row is dropped, on the
CPU and in advance, when the oracle does not solve it, when its oracle slope dp/dT is not positive, or when the oracle does
not solve it at 0.93 or 1.07 T_grid (the displaced starts must be meaningful).  At most CAP of the rows of any
(class, factor, problem) cell may be dropped; the committed SEED and FACTORS meet that (tests/test_mix_temperature_referee.py).
"""
import numpy as np

N_ROWS, SEED = 192, 2024
FACTORS = (0.85, 1.0, 1.2)
STARTS = (1.0, 0.93, 1.07)  # first iterates, as factors of T_grid
CAP = 0.10
N_CLASSES = 6


class Inputs:
    pass


def solve_temperature(orc, P, K, z, p_spec, T0, dew, tol=1e-14, max_it=60):
    """-> T [n] (NaN where the referee fails), p [n] the oracle's pressure at T, rho4 [n,4] at T.  Vectorised over the rows;
    every row keeps its own bracket."""
    n = len(T0)
    ln_ps = np.log(p_spec)
    x = 1.0 / np.asarray(T0, dtype=np.float64)
    p_start = np.array(p_spec, dtype=np.float64)
    x_lo = np.full(n, np.inf)   # x of the highest T with f < 0 (x_hi < x < x_lo)
    x_hi = np.zeros(n)          # x of the lowest T with f > 0
    xp, fp = np.full(n, np.nan), np.full(n, np.nan)
    T_out, p_out, rho_out = np.full(n, np.nan), np.full(n, np.nan), np.full((n, 4), np.nan)
    live = np.ones(n, dtype=bool)
    for _ in range(max_it):
        idx = np.nonzero(live)[0]
        if len(idx) == 0:
            break
        p, rho4, st = orc.mix_bubble_dew(P[idx], K[idx], 1.0 / x[idx], z[idx], p_start[idx], dew, prec=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            f = np.log(p) - ln_ps[idx]
        bad = st | ~np.isfinite(f)
        live[idx[bad]] = False  # no equilibrium at a trial: the referee gives the row up (NaN)
        idx, f, p, rho4 = idx[~bad], f[~bad], p[~bad], rho4[~bad]
        p_start[idx] = p
        neg = f < 0
        x_lo[idx[neg]] = np.minimum(x_lo[idx[neg]], x[idx[neg]])
        x_hi[idx[~neg]] = np.maximum(x_hi[idx[~neg]], x[idx[~neg]])
        # secant through the last two trials; the first step assumes d ln p / d ln T = 10
        with np.errstate(invalid="ignore", divide="ignore"):
            slope = (f - fp[idx]) / (x[idx] - xp[idx])
        first = ~np.isfinite(slope) | (slope >= 0)
        slope = np.where(first, -10.0 / x[idx], slope)
        x_new = x[idx] - f / slope
        lo, hi = x_lo[idx], x_hi[idx]
        bracketed = np.isfinite(lo) & (hi > 0)
        outside = ~((x_new > hi) & (x_new < lo))
        x_new = np.where(bracketed & outside, 0.5 * (lo + hi), x_new)
        x_new = np.where(~bracketed, np.clip(x_new, x[idx] / 1.15, x[idx] * 1.15), x_new)
        conv = (np.abs(f) <= tol) | (np.abs(x_new - x[idx]) <= 1e-16 * x[idx])
        done = idx[conv]
        T_out[done], p_out[done], rho_out[done] = 1.0 / x[done], p[conv], rho4[conv]
        live[done] = False
        xp[idx], fp[idx] = x[idx], f
        x[idx] = x_new
    return T_out, p_out, rho_out


def quotient(grad):
    """[n,19] gradient of the pressure w.r.t. (16 parameters, kij0, kij1, T) -> [n,19] gradient of the temperature w.r.t.
    (16 parameters, kij0, kij1, p_spec)."""
    inv = 1.0 / grad[:, 18:19]
    return np.concatenate((-grad[:, :18] * inv, inv), axis=1)


def gradient(orc, P, K, T, rho4, dew, exact=True):
    return quotient(orc.mix_bubble_dew_grad(P, K, T, rho4, dew, exact=exact)[1])


_CACHE = {}


def inputs(orc, dew):
    """The input set of one problem: 3 x 192 rows, factor-major.  Cached per process."""
    if dew in _CACHE:
        return _CACHE[dew]
    from feos_torch_amd.synthetic import mix_batch

    P, K, T, X, PI = mix_batch(N_ROWS, SEED)
    c = Inputs()
    nf = len(FACTORS)
    c.n = n = nf * N_ROWS
    c.P, c.K, c.z = np.tile(P, (nf, 1, 1)), np.tile(K, (nf, 1)), np.tile(X, nf)
    c.T = np.concatenate([s * T for s in FACTORS])
    c.cls = np.tile(np.arange(N_ROWS) % N_CLASSES, nf)
    c.factor = np.repeat(np.arange(nf), N_ROWS)
    c.cell = c.factor * N_CLASSES + c.cls
    p, rho4, st = orc.mix_bubble_dew(c.P, c.K, c.T, c.z, np.tile(PI, nf), dew, prec=1)
    ok = ~st & np.isfinite(p) & (p > 0)
    c.p_spec = np.where(ok, p, 1e5)  # rows the oracle does not solve stay in the batch as wave mates
    c.rho4 = np.where(ok[:, None], rho4, np.nan)
    safe = np.where(ok[:, None], rho4, np.array([1e-6, 1e-6, 5e-3, 5e-3]))
    c.grad = orc.mix_bubble_dew_grad(c.P, c.K, c.T, safe, dew, exact=True)[1]
    c.grad64 = orc.mix_bubble_dew_grad(c.P, c.K, c.T, safe, dew, exact=False)[1]
    with np.errstate(invalid="ignore", divide="ignore"):
        c.dlnp_dlnT = c.grad[:, 18] * c.T / c.p_spec
    ok &= np.isfinite(c.dlnp_dlnT) & (c.grad[:, 18] > 0)
    # the displaced starts: the oracle must have an equilibrium there too; the solutions also give d ln rho / d ln p along the line
    c.side = {}
    for s in STARTS[1:]:
        ps, rs, sts = orc.mix_bubble_dew(c.P, c.K, s * c.T, c.z, c.p_spec, dew, prec=1)
        ok &= ~sts & np.isfinite(ps) & (ps > 0)
        c.side[s] = (ps, rs)
    c.keep = ok
    (p_a, r_a), (p_b, r_b) = c.side[STARTS[1]], c.side[STARTS[2]]
    with np.errstate(invalid="ignore", divide="ignore"):
        c.dlnrho_dlnp = np.abs(np.log(r_b / r_a)).max(axis=1) / np.abs(np.log(p_b / p_a))
    c.dropped_share = np.array([np.mean(~c.keep[c.cell == k]) for k in range(nf * N_CLASSES)])
    _CACHE[dew] = c
    return c


def per_cell_max(c, values, mask):
    """[n]: for every row the largest of values[mask] over the row's (class, factor) cell (0 where the cell has none)"""
    out = np.zeros(c.n)
    for k in np.unique(c.cell):
        m = (c.cell == k) & mask
        if m.any():
            out[c.cell == k] = np.nanmax(values[m])
    return out


def interleave(n):
    """a fixed permutation that mixes the factor blocks: position -> row"""
    return np.arange(n).reshape(len(FACTORS), -1).T.ravel()
