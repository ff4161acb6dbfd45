"""Referee and input set for GcPcSaftMix.vapor_pressure / equilibrium_liquid_density (test infrastructure, numpy + oracle only).
It takes none of the kernel's decisions.

Solve.  Molecule `comp` of a row taken as a pure fluid is the oracle's model at the partial densities (rho, 0) (comp 0) or
(0, rho) (comp 1): a, p and the residual chemical potential mu = da/drho of that component come from
oracle.gc_derivatives(prec=1), long double rounded to double on return (Rows, packing and line of gc_density_referee are
reused).  The pure line is scanned on the FIXED grid ETA of packing fractions, 0.5 down to 0.005 in steps of 0.005 and then
halved twenty times.  Going down from 0.5 the pressure must fall (a liquid branch exists there); the first grid point behind
which it rises again is the liquid spinodal's, the first one behind which it falls again the vapour spinodal's: that is the
van der Waals loop.  No first turn means no loop (T at or above the critical temperature), a non-positive pressure at the
second one means no equilibrium either.  The liquid is bracketed between its spinodal point and eta = 0.74, the vapour between
0 and its spinodal point; both start from the branch roots of p = mean of the two spinodal pressures (the negative one taken
as 0).  Then Newton on
    F = (p_V - p_L,  (mu_V + ln rho_V) - (mu_L + ln rho_L)) = 0,     J = [[p'_V, -p'_L], [p'_V / rho_V, -p'_L / rho_L]]
(p' = dp/drho from the central difference of `line`; it only steers the step), steps halved until both densities stay inside
their brackets, to a relative step of 1e-15 -- or, since mu + ln rho is a double of magnitude ~15, until the step has stopped
shrinking below 1e-13.  p_sat is the equal-area formula at the result,
    p* = -(a_V / rho_V - a_L / rho_L + ln(rho_V / rho_L)) / dv,   dv = 1 / rho_V - 1 / rho_L,   p_sat [Pa] = p* T k_B 1e30.
The fp64 twin is the same solve with prec=0 (the oracle's fp64 evaluation, safeguarded association); it sets the bars.

Exact slopes and gradients: oracle.gc_derivatives_vjp_exact with weights on a and p only.  gp = 1 at a root gives the row's
dp/d(phi_0, phi_1, T, rho_0, rho_1); the density column of the component is the slope p' at the root.  With @ a partial
derivative at fixed densities and theta any parameter:
    p* is stationary in both densities, so  dp*/dtheta = -(@a_V/@theta / rho_V - @a_L/@theta / rho_L) / dv:
        for an upstream gradient g of p_sat [Pa], w = g T k_B 1e30: ga = -w / (rho_V dv) at the vapour, ga = +w / (rho_L dv) at
        the liquid, and d p_sat/dT has the explicit term g p_sat / T on top of the two T columns;
    rho_L is defined by p_L(rho_L, theta) = p*(theta), so  d rho_L/dtheta = (dp*/dtheta - @p_L/@theta) / p'_L:
        the same with w = g / p'_L, and gp = -g / p'_L at the liquid; no explicit T term (both are reduced pressures of one T).
The k_ab and segment-table sums are the oracle's own sums of the two calls (table entries: Richardson differences).

Input set (the GPU test uses the same).  The 384 gc rows of gc_temperature_referee.inputs, both components.  For each (row,
component) T_top is the highest temperature of the ladder 120 K x 1.04^k, k = 0 .. 60, at which this referee finds the
equilibrium (searched on every tenth rung, then by bisection between the highest solved rung and the next one).  The batch is
T = FACTORS x T_top, component-major, then factor, then row: 3,072 rows.  A row is kept when the referee solves it and the
reduced dp/drho at both roots is >= MIN_SLOPE, the rule of the density referee.  At most CAP of the rows of any (class,
component, factor) cell may be dropped (tests/test_gc_saturation_referee.py); the FACTORS of the issue meet that unchanged.
"""
import numpy as np

import gc_density_referee as dref
import gc_temperature_referee as tref

from gc_density_referee import Rows, line, packing  # noqa: F401  (the helpers this referee reuses)

N_ROWS = tref.N_ROWS
FACTORS = (0.55, 0.70, 0.85, 0.95)
LADDER = 120.0 * 1.04 ** np.arange(61)
MIN_SLOPE = dref.MIN_SLOPE
CAP = 0.10
D_ETA = 0.005
ETA = np.concatenate((0.5 - D_ETA * np.arange(100), 0.005 * 0.5 ** np.arange(1, 21)))
ETA_MAX = 0.74
FD_STEP = dref.FD_STEP
P_RED = dref.P_RED  # p* = p [Pa] P_RED / T
C_UNIT = 1.0 / (1e3 * (6.02214076e23 * (1e-10 * 1e-10 * 1e-10)))  # A^-3 -> kmol/m3
SEED = 2046


def _r2(comp, rho):
    out = np.zeros((len(rho), 2))
    out[np.arange(len(rho)), comp] = rho
    return out


def evaluate(m, idx, comp, T, rho, prec=1):
    """a, p, mu (of the component) [n] at the total densities rho of the pure fluid"""
    enc, phi = m.sub(idx)
    a, p, mu, _ = m.orc.gc_derivatives(enc, phi, T, _r2(comp, rho), robust=True, prec=prec)
    return a, p, mu[np.arange(len(rho)), comp]


def slope(m, idx, comp, T, rho, prec=1):
    """central-difference dp/drho [n]: `line` of the density referee in long double, the same difference in fp64 for the twin"""
    if prec == 1:
        return line(m, idx, T, 1.0 - comp, rho)[1]
    hi = evaluate(m, idx, comp, T, rho * (1.0 + FD_STEP), prec)[1]
    lo = evaluate(m, idx, comp, T, rho * (1.0 - FD_STEP), prec)[1]
    return (hi - lo) / (2.0 * FD_STEP * rho)


def _branch(m, idx, comp, T, target, lo, hi, rho, prec, tol=1e-10, max_it=100):
    """root of p = target in [lo, hi] on a branch on which p rises with rho: Newton inside the bracket, else bisection"""
    lo, hi, rho = lo.copy(), hi.copy(), rho.copy()
    done = np.zeros(len(T), dtype=bool)
    for _ in range(max_it):
        k = np.nonzero(~done)[0]
        if len(k) == 0:
            break
        p = evaluate(m, idx[k], comp[k], T[k], rho[k], prec)[1]
        s = slope(m, idx[k], comp[k], T[k], rho[k], prec)
        f = p - target[k]
        lo[k] = np.where(f < 0, rho[k], lo[k])
        hi[k] = np.where(f < 0, hi[k], rho[k])
        with np.errstate(invalid="ignore", divide="ignore"):
            new = rho[k] - f / s
        inside = np.isfinite(new) & (new > lo[k]) & (new < hi[k]) & (s > 0)
        new = np.where(inside, new, 0.5 * (lo[k] + hi[k]))
        conv = np.abs(new - rho[k]) <= tol * rho[k]
        rho[k] = new
        done[k[conv]] = True
    return rho, done


def equal_area(a_v, a_l, rho_v, rho_l):
    return -(a_v / rho_v - a_l / rho_l + np.log(rho_v / rho_l)) / (1.0 / rho_v - 1.0 / rho_l)


def solve(m, idx, comp, T, prec=1):
    """-> dict(ok [n] bool, rho_v, rho_l [A^-3], p_star (reduced), p_sat [Pa], f1, f2 (the residuals F at the result, f1 relative
    to max(p*, p'_L rho_L): one ulp of rho_L moves p_L by p'_L rho_L 1e-16), steps); NaN where not ok.  Vectorised; idx: rows of m."""
    idx, comp, T = np.asarray(idx), np.asarray(comp), np.asarray(T, dtype=np.float64)
    n = len(T)
    nan = lambda: np.full(n, np.nan)
    out = {"ok": np.zeros(n, dtype=bool), "rho_v": nan(), "rho_l": nan(), "p_star": nan(), "p_sat": nan(), "f1": nan(), "f2": nan()}
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(T) & (T > 0)
    v = np.nonzero(valid)[0]
    if len(v) == 0:
        return out
    iv, cv, Tv = idx[v], comp[v], T[v]
    pk = packing(m.enc, iv, Tv, 1.0 - cv)
    nv = len(v)
    P = np.stack([evaluate(m, iv, cv, Tv, eta / pk, prec)[1] for eta in ETA], axis=1)  # [nv, G]
    rises = ~(np.diff(P, axis=1) < 0)  # going down in density the pressure does not fall: behind a spinodal (or not finite)
    G = len(ETA)
    first = lambda mask: np.where(mask.any(axis=1), mask.argmax(axis=1), G)
    jl = first(rises)  # grid point of the liquid spinodal
    after = np.arange(G - 1)[None, :] > jl[:, None]
    jv = first(~rises & after)  # grid point of the vapour spinodal
    live = (jl >= 1) & (jl < G) & (jv < G) & np.isfinite(P).all(axis=1)
    rows = np.arange(nv)
    p_min = P[rows, np.minimum(jl, G - 1)]
    p_max = P[rows, np.minimum(jv, G - 1)]
    live &= p_max > 0
    k = np.nonzero(live)[0]
    if len(k) == 0:
        return out
    ik, ck, Tk, pkk = iv[k], cv[k], Tv[k], pk[k]
    lo_l, hi_l = ETA[jl[k]] / pkk, np.full(len(k), ETA_MAX) / pkk
    lo_v, hi_v = np.zeros(len(k)), ETA[jv[k]] / pkk
    p0 = 0.5 * (np.maximum(p_min[k], 0.0) + p_max[k])
    rl, ok_l = _branch(m, ik, ck, Tk, p0, lo_l, hi_l, ETA[jl[k] - 1] / pkk, prec)
    rv, ok_v = _branch(m, ik, ck, Tk, p0, lo_v, hi_v, np.minimum(p0, 0.5 * hi_v), prec)
    good = ok_l & ok_v
    done = np.zeros(len(k), dtype=bool)
    prev = np.full(len(k), np.inf)
    f1, f2 = np.full(len(k), np.nan), np.full(len(k), np.nan)
    for it in range(80):
        q = np.nonzero(good & ~done)[0]
        if len(q) == 0:
            break
        a_v, p_v, mu_v = evaluate(m, ik[q], ck[q], Tk[q], rv[q], prec)
        a_l, p_l, mu_l = evaluate(m, ik[q], ck[q], Tk[q], rl[q], prec)
        s_v, s_l = slope(m, ik[q], ck[q], Tk[q], rv[q], prec), slope(m, ik[q], ck[q], Tk[q], rl[q], prec)
        F1 = p_v - p_l
        F2 = (mu_v + np.log(rv[q])) - (mu_l + np.log(rl[q]))
        dv = 1.0 / rv[q] - 1.0 / rl[q]
        with np.errstate(invalid="ignore", divide="ignore"):
            d_v = (F1 / rl[q] - F2) / (s_v * dv)
            d_l = (F1 / rv[q] - F2) / (s_l * dv)
        sane = np.isfinite(d_v) & np.isfinite(d_l) & (s_v > 0) & (s_l > 0)
        good[q[~sane]] = False
        for _ in range(40):  # both densities stay inside their brackets
            nv_, nl_ = rv[q] + d_v, rl[q] + d_l
            out_ = sane & ~((nv_ > lo_v[q]) & (nv_ < hi_v[q]) & (nl_ > lo_l[q]) & (nl_ < hi_l[q]))
            if not out_.any():
                break
            d_v, d_l = np.where(out_, 0.5 * d_v, d_v), np.where(out_, 0.5 * d_l, d_l)
        with np.errstate(invalid="ignore"):
            step = np.maximum(np.abs(d_v) / rv[q], np.abs(d_l) / rl[q])
        f1[q] = F1 / np.maximum(np.abs(p_v), s_l * rl[q])
        f2[q] = F2
        conv = sane & ((step <= 1e-15) | ((it >= 5) & (step <= 1e-13) & (step >= 0.25 * prev[q])))
        prev[q] = step
        upd = sane & ~conv  # the result is the point the residuals were taken at
        rv[q] = np.where(upd, rv[q] + d_v, rv[q])
        rl[q] = np.where(upd, rl[q] + d_l, rl[q])
        done[q[conv]] = True
    fin = np.nonzero(good & done & (rv < rl * (1.0 - 1e-6)))[0]
    if len(fin) == 0:
        return out
    a_v = evaluate(m, ik[fin], ck[fin], Tk[fin], rv[fin], prec)[0]
    a_l = evaluate(m, ik[fin], ck[fin], Tk[fin], rl[fin], prec)[0]
    ps = equal_area(a_v, a_l, rv[fin], rl[fin])
    pos = ps > 0
    fin, ps = fin[pos], ps[pos]
    at = v[k[fin]]
    out["ok"][at] = True
    out["rho_v"][at], out["rho_l"][at] = rv[fin], rl[fin]
    out["p_star"][at], out["p_sat"][at] = ps, ps * Tk[fin] / P_RED
    out["f1"][at], out["f2"][at] = f1[fin], f2[fin]
    return out


def exact(m, idx, comp, T, rho, ga, gp):
    """gc_derivatives_vjp_exact at the pure state with weights on a and p only -> grad_row [n,5], grad_seg [S,8], grad_kab [S,S]"""
    enc, phi = m.sub(idx)
    z2 = np.zeros((len(T), 2))
    return m.orc.gc_derivatives_vjp_exact(enc, phi, T, _r2(comp, rho), ga, gp, z2, z2)


def slopes(m, idx, comp, T, rho):
    """exact dp/drho along the pure line at rho"""
    n = len(T)
    grow = exact(m, idx, comp, T, rho, np.zeros(n), np.ones(n))[0]
    return grow[np.arange(n), 3 + comp]


def gradient(m, idx, comp, T, rho_v, rho_l, p_sat, dp_l, g, which):
    """The formulas of the module docstring for an upstream gradient g [n] of p_sat [Pa] (which 0) or rho_L [A^-3] (which 1):
    -> row [n,3] = g d value / d(phi_0, phi_1, T), grad_seg [S,8], grad_kab [S,S] (the sums over the rows)."""
    n = len(T)
    dv = 1.0 / rho_v - 1.0 / rho_l
    w = g * T / P_RED if which == 0 else g / dp_l
    gp_l = np.zeros(n) if which == 0 else -w
    row_v, seg_v, kab_v = exact(m, idx, comp, T, rho_v, -w / (rho_v * dv), np.zeros(n))
    row_l, seg_l, kab_l = exact(m, idx, comp, T, rho_l, w / (rho_l * dv), gp_l)
    row = row_v[:, :3] + row_l[:, :3]
    if which == 0:
        row[:, 2] += g * p_sat / T
    return row, seg_v + seg_l, kab_v + kab_l


class Inputs:
    pass


_CACHE = {}


def t_top(m, idx, comp):
    """[n] highest rung of LADDER at which `solve` finds the equilibrium (NaN: none)"""
    n = len(idx)
    coarse = np.arange(0, len(LADDER), 10)
    ok = np.stack([solve(m, idx, comp, np.full(n, LADDER[k]))["ok"] for k in coarse], axis=1)
    any_ok = ok.any(axis=1)
    last = np.where(any_ok, ok.shape[1] - 1 - ok[:, ::-1].argmax(axis=1), 0)
    lo = coarse[last]                                   # solved (where any_ok)
    hi = np.minimum(lo + 10, len(LADDER))               # not solved, or past the ladder
    while True:
        open_ = np.nonzero(any_ok & (hi - lo > 1))[0]
        if len(open_) == 0:
            break
        mid = (lo[open_] + hi[open_]) // 2
        good = solve(m, idx[open_], comp[open_], LADDER[mid])["ok"]
        lo[open_] = np.where(good, mid, lo[open_])
        hi[open_] = np.where(good, hi[open_], mid)
    return np.where(any_ok, LADDER[lo], np.nan)


def base_rows(orc):
    b = tref.inputs(orc, False)
    first = np.arange(N_ROWS)
    enc, phi = tref.sub_enc(b.enc, first), np.ascontiguousarray(b.phi[:N_ROWS])
    return b, Rows(orc, enc, phi)


def inputs(orc):
    """The input set: 2 components x 4 factors x 384 rows, with the referee's solution, its fp64 twin and the exact slopes."""
    if "inputs" in _CACHE:
        return _CACHE["inputs"]
    b, m = base_rows(orc)
    c = Inputs()
    c.base, c.m = b, m
    c.segment_lists, c.bond_lists, c.kab_list = b.segment_lists[:N_ROWS], b.bond_lists[:N_ROWS], b.kab_list
    r1 = np.arange(N_ROWS)
    c.t_top = np.stack([t_top(m, r1, np.full(N_ROWS, k)) for k in (0, 1)])  # [2, 384]
    nf = len(FACTORS)
    c.n = 2 * nf * N_ROWS
    c.row = np.tile(r1, 2 * nf)
    c.comp = np.repeat(np.arange(2), nf * N_ROWS)
    c.factor = np.tile(np.repeat(np.arange(nf), N_ROWS), 2)
    top = c.t_top[c.comp, c.row]
    c.has_top = np.isfinite(top)
    c.T = np.where(c.has_top, np.array(FACTORS)[c.factor] * np.where(c.has_top, top, 1.0), 300.0)
    c.T_top = np.where(c.has_top, top, 300.0 / 1.5)
    c.phi = m.phi[c.row]
    c.cls = b.cls[:N_ROWS][c.row]
    c.classes = np.unique(c.cls)
    c.cell = (c.cls * 2 + c.comp) * nf + c.factor
    c.cells = np.unique(c.cell)
    c.sol = solve(m, c.row, c.comp, c.T)
    c.twin = solve(m, c.row, c.comp, c.T, prec=0)
    ok = c.sol["ok"] & c.has_top
    c.rho_v, c.rho_l, c.p_sat = c.sol["rho_v"], c.sol["rho_l"], c.sol["p_sat"]
    c.dp_v, c.dp_l = np.full(c.n, np.nan), np.full(c.n, np.nan)
    c.dp_v64, c.dp_l64 = np.full(c.n, np.nan), np.full(c.n, np.nan)
    k = np.nonzero(ok)[0]
    c.dp_v[k] = slopes(m, c.row[k], c.comp[k], c.T[k], c.rho_v[k])
    c.dp_l[k] = slopes(m, c.row[k], c.comp[k], c.T[k], c.rho_l[k])
    k2 = np.nonzero(ok & c.twin["ok"])[0]  # the twin's slopes: the exact slope function at the twin's own roots
    c.dp_v64[k2] = slopes(m, c.row[k2], c.comp[k2], c.T[k2], c.twin["rho_v"][k2])
    c.dp_l64[k2] = slopes(m, c.row[k2], c.comp[k2], c.T[k2], c.twin["rho_l"][k2])
    with np.errstate(invalid="ignore"):
        c.keep = ok & (c.dp_v >= MIN_SLOPE) & (c.dp_l >= MIN_SLOPE)
    c.dropped_share = {int(q): float(np.mean(~c.keep[c.cell == q])) for q in c.cells}
    for val in list(vars(c).values()) + list(c.sol.values()) + list(c.twin.values()):
        if isinstance(val, np.ndarray):
            val.setflags(write=False)
    _CACHE["inputs"] = c
    return c


def twin_error(c):
    """{name: [n]} relative error of the fp64 twin against the long-double solve on the kept rows (NaN elsewhere, and where the
    twin fails): what the bars of the GPU test are made of"""
    with np.errstate(invalid="ignore"):
        e = {"p_sat": np.abs(c.twin["p_sat"] / c.p_sat - 1.0), "rho_v": np.abs(c.twin["rho_v"] / c.rho_v - 1.0),
             "rho_l": np.abs(c.twin["rho_l"] / c.rho_l - 1.0), "dp_v": np.abs(c.dp_v64 / c.dp_v - 1.0), "dp_l": np.abs(c.dp_l64 / c.dp_l - 1.0)}
    return {k: np.where(c.keep, v, np.nan) for k, v in e.items()}


def weighted(orc, c, which, comp):
    """The referee of the gradient test, once per (output, component): seeded upstream gradients g ~ U(0.5, 1.5) of the output in
    the kernel's units (Pa, A^-3) on the kept rows of the component, and per model class (the weights masked to it) the
    gradient sums: {'g': [n], 'groups': {class: dict(rows, row [m,3], grad_kab, grad_seg)}, 'all': sums over the classes}."""
    key = ("weighted", which, comp)
    if key not in _CACHE:
        g = np.where(c.keep & (c.comp == comp), np.random.default_rng(SEED + 2 * which + comp).uniform(0.5, 1.5, c.n), 0.0)
        out = {"g": g, "groups": {}}
        S = c.m.enc["S"]
        tot = {"grad_kab": np.zeros((S, S)), "grad_seg": np.zeros((S, 8))}
        for k in c.classes:
            rows = np.nonzero(c.keep & (c.comp == comp) & (c.cls == k))[0]
            if len(rows) == 0:
                continue
            row, gseg, gkab = gradient(c.m, c.row[rows], c.comp[rows], c.T[rows], c.rho_v[rows], c.rho_l[rows], c.p_sat[rows],
                                       c.dp_l[rows], g[rows], which)
            out["groups"][int(k)] = {"rows": rows, "row": row, "grad_kab": gkab, "grad_seg": gseg}
            tot["grad_kab"] += gkab
            tot["grad_seg"] += gseg
        out["all"] = tot
        _CACHE[key] = out
    return _CACHE[key]


def interleave(n):
    """a fixed permutation that mixes components, temperature factors and classes within a wave: position -> row"""
    return np.arange(n).reshape(2 * len(FACTORS), -1).T.ravel()
