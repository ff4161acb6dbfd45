"""Brute-force referee of the tangent-plane stability analysis (CPU, oracle only; independent of the kernels' search).

For every feed (T, partial densities rho^f) it evaluates tpd = sum_i w_i (mu_i(rho^t) - mu_i(rho^f)) at EVERY mechanically
stable density root rho^t of p(w rho) = p^f on a fixed grid of trial compositions w (logit-spaced, plus caller-supplied ones)
and returns the smallest non-trivial value.  Roots: a scan in packing fraction (geometric up to 0.1, linear above) for
upward crossings of p^f, each polished by a bracketed secant (Illinois) iteration in ln rho to the rounding floor.  Definitions
as in include/pcsaft_hip.h (pcs_mix_stability).

`derivs(rows, rho)` -> (a, p, mu_res, v) of the oracle for feed indices `rows` at partial densities rho [m,2] (reduced);
`pk` [F,2]: packing fraction per unit density of each pure component (pi/6 m d^3).
"""
import numpy as np

TPD_TOL = 1e-8
TRIVIAL = 1e-6


def mix_derivs(orc, params, kij, T):
    return lambda rows, rho: orc.mix_derivatives(params[rows], kij[rows], T[rows], rho, robust=True)


def gc_derivs(orc, enc, phi, T):
    def f(rows, rho):
        e = dict(enc)
        e["counts"] = enc["counts"][rows]
        e["bonds"] = enc["bonds"][rows]
        return orc.gc_derivatives(e, phi[rows], T[rows], rho, robust=True)

    return f


def mix_packing(params, T):
    """[F,2] pi/6 m d^3 of the two components (d = sigma (1 - 0.12 exp(-3 eps/T)))."""
    m, s, e = params[:, :, 0], params[:, :, 1], params[:, :, 2]
    d = s * (1.0 - 0.12 * np.exp(-3.0 * e / T[:, None]))
    return np.pi / 6.0 * m * d**3


def gc_packing(enc, T):
    seg = enc["seg"]
    d = seg[None, :, 1] * (1.0 - 0.12 * np.exp(-3.0 * seg[None, :, 2] / T[:, None]))  # [F,S]
    return np.pi / 6.0 * np.einsum("fcs,fs->fc", enc["counts"], seg[None, :, 0] * d**3)


def composition_grid(nw=128, lo=1e-8):
    s = np.linspace(np.log(lo / (1.0 - lo)), np.log((1.0 - lo) / lo), nw)
    return 1.0 / (1.0 + np.exp(-s))


def _eval_chunks(derivs, rows, rho, chunk=400000):
    p = np.empty(len(rows))
    mu = np.empty((len(rows), 2))
    for k in range(0, len(rows), chunk):
        _, pp, mm, _ = derivs(rows[k:k + chunk], rho[k:k + chunk])
        p[k:k + chunk] = pp
        mu[k:k + chunk] = mm
    return p, mu


def feed_state(derivs, rho_f):
    F = len(rho_f)
    _, p, mu, _ = derivs(np.arange(F), rho_f)
    return p, np.log(rho_f) + mu


def roots(derivs, pk, rho_f, pf, w, n_geo=60, n_lin=100, iters=60):
    """All upward crossings of p^f along each trial composition.  w [F,G].  -> (feed index, composition w_1, total
    density) of every root, each array [R]."""
    F, G = w.shape
    pkw = w * pk[:, 0:1] + (1.0 - w) * pk[:, 1:2]  # [F,G]
    eta_lo = np.minimum(0.3 * np.abs(pf[:, None]) * pkw.min(axis=1, keepdims=True), 1e-2)  # below the ideal-gas density
    eta_lo = np.where(eta_lo > 1e-300, eta_lo, 1e-300)
    geo = np.exp(np.log(eta_lo) + np.linspace(0.0, 1.0, n_geo)[None, :] * (np.log(0.1) - np.log(eta_lo)))  # [F,n_geo]
    eta = np.concatenate([geo[:, :-1], np.broadcast_to(np.linspace(0.1, 0.74, n_lin)[None, :], (F, n_lin))], axis=1)  # [F,E]
    E = eta.shape[1]
    rho = eta[:, None, :] / pkw[:, :, None]  # [F,G,E]
    rows = np.broadcast_to(np.arange(F)[:, None, None], rho.shape).ravel()
    ww = np.broadcast_to(w[:, :, None], rho.shape).ravel()
    rr = rho.ravel()
    p, _ = _eval_chunks(derivs, rows, np.stack([ww * rr, (1.0 - ww) * rr], axis=1))
    g = (p.reshape(F, G, E) - pf[:, None, None])
    up = (g[:, :, :-1] < 0.0) & (g[:, :, 1:] > 0.0)
    fi, gi, ei = np.nonzero(up)
    xa, xb = np.log(rho[fi, gi, ei]), np.log(rho[fi, gi, ei + 1])
    ga, gb = g[fi, gi, ei], g[fi, gi, ei + 1]
    wr = w[fi, gi]
    side = np.zeros(len(fi), dtype=np.int8)
    active = np.ones(len(fi), dtype=bool)
    for _ in range(iters):
        k = np.nonzero(active)[0]
        if len(k) == 0:
            break
        xc = xb[k] - gb[k] * (xb[k] - xa[k]) / (gb[k] - ga[k])
        bad = ~((xc > xa[k]) & (xc < xb[k]))
        xc[bad] = 0.5 * (xa[k][bad] + xb[k][bad])
        r = np.exp(xc)
        pc, _ = _eval_chunks(derivs, fi[k], np.stack([wr[k] * r, (1.0 - wr[k]) * r], axis=1))
        gc = pc - pf[fi[k]]
        lowside = gc < 0.0
        a_k, b_k = k[lowside], k[~lowside]
        xa[a_k], ga[a_k] = xc[lowside], gc[lowside]
        gb[a_k[side[a_k] == -1]] *= 0.5
        side[a_k] = -1
        xb[b_k], gb[b_k] = xc[~lowside], gc[~lowside]
        ga[b_k[side[b_k] == 1]] *= 0.5
        side[b_k] = 1
        done = (xb[k] - xa[k] <= 4e-16 * np.abs(xb[k]) + 1e-300) | (gc == 0.0)
        active[k[done]] = False
    x = np.where(np.abs(ga) < np.abs(gb), xa, xb)
    return fi, wr, np.exp(x)


def tpd_minimum(derivs, pk, rho_f, extra_w=None, nw=128):
    """-> dict(tpd [F] smallest non-trivial tpd (+inf: no non-trivial root), trial [F,2] its partial densities, pf [F],
    mu_f [F,2], roots (fi, w, rho, tpd) of every root)."""
    rho_f = np.ascontiguousarray(rho_f, dtype=np.float64)
    F = len(rho_f)
    pf, muf = feed_state(derivs, rho_f)
    w = np.broadcast_to(composition_grid(nw)[None, :], (F, nw))
    if extra_w is not None:
        w = np.concatenate([w, np.asarray(extra_w, dtype=np.float64).reshape(F, -1)], axis=1)
    fi, wr, rt = roots(derivs, pk, rho_f, pf, np.ascontiguousarray(w))
    rho_t = np.stack([wr * rt, (1.0 - wr) * rt], axis=1)
    keep = np.all(rho_t > 0.0, axis=1)
    fi, wr, rt, rho_t = fi[keep], wr[keep], rt[keep], rho_t[keep]
    _, mu = _eval_chunks(derivs, fi, rho_t)
    tpd = wr * (np.log(rho_t[:, 0]) + mu[:, 0] - muf[fi, 0]) + (1.0 - wr) * (np.log(rho_t[:, 1]) + mu[:, 1] - muf[fi, 1])
    rf = rho_f.sum(axis=1)
    z = rho_f[:, 0] / rf
    trivial = (np.abs(wr - z[fi]) < TRIVIAL) & (np.abs(rt / rf[fi] - 1.0) < TRIVIAL)
    best = np.full(F, np.inf)
    trial = np.full((F, 2), np.nan)
    ok = ~trivial & np.isfinite(tpd)
    order = np.lexsort((tpd[ok], fi[ok]))  # per feed ascending tpd
    fo = fi[ok][order]
    first = np.ones(len(fo), dtype=bool)
    first[1:] = fo[1:] != fo[:-1]
    sel = np.nonzero(ok)[0][order][first]
    best[fi[sel]] = tpd[sel]
    trial[fi[sel]] = rho_t[sel]
    return {"tpd": best, "trial": trial, "pf": pf, "mu_f": muf, "roots": (fi, wr, rt, tpd)}


def recompute(derivs, rows, rho_f, rho_t):
    """(p^f, p(rho^t), tpd) recomputed at given trial partial densities: the check of a reported trial phase."""
    pf, muf = feed_state(lambda r, x: derivs(rows[r], x), rho_f)
    _, pt, mut, _ = derivs(rows, rho_t)
    w = rho_t / rho_t.sum(axis=1, keepdims=True)
    tpd = (w * (np.log(rho_t) + mut - muf)).sum(axis=1)
    return pf, pt, tpd


def liquid_root(derivs, pk, z, p, vapour=False):
    """Densest (vapour=True: most dilute) mechanically stable root of p(z rho) = p at a given composition and reduced
    pressure [F] (NaN: none)."""
    F = len(z)
    rho_f = np.stack([z * 1e-3, (1.0 - z) * 1e-3], axis=1)  # only its composition enters roots()
    fi, wr, rt = roots(derivs, pk, rho_f, np.asarray(p, dtype=np.float64), np.asarray(z, dtype=np.float64).reshape(F, 1))
    out = np.full(F, np.nan)
    (np.fmin if vapour else np.fmax).at(out, fi, rt)
    return out


def hessian_det(derivs, rho, h=1e-6):
    """det of the Hessian of a + sum rho_i (ln rho_i - 1) in the partial densities (central differences of mu)."""
    rho = np.asarray(rho, dtype=np.float64)
    F = len(rho)
    H = np.empty((F, 2, 2))
    for j in range(2):
        d = np.zeros_like(rho)
        d[:, j] = h * rho[:, j]
        _, _, mp, _ = derivs(np.arange(F), rho + d)
        _, _, mm, _ = derivs(np.arange(F), rho - d)
        H[:, :, j] = (np.log(rho + d) + mp - np.log(rho - d) - mm) / (2.0 * d[:, j:j + 1])
    return H[:, 0, 0] * H[:, 1, 1] - H[:, 0, 1] * H[:, 1, 0]


def is_root(derivs, rows, pf, rho_t, noise=0.0, rel=1e-12):
    """rho^t is a root of p = p^f: |p(rho^t) - p^f| <= 1e-9 p^f + `noise` (the measured rounding error of the double-precision
    pressures: see mix_pressure_noise), or within what a relative change of `rel` in the density moves the pressure (a dense
    phase at a very low pressure: one rounding step of the density changes p by more than 1e-9 p^f)."""
    rho_t = np.asarray(rho_t, dtype=np.float64)
    _, p0, _, _ = derivs(rows, rho_t)
    _, p1, _, _ = derivs(rows, rho_t * (1.0 + rel))
    _, p2, _, _ = derivs(rows, rho_t * (1.0 - rel))
    return np.abs(p0 - pf) <= 1e-9 * np.abs(pf) + noise + 0.5 * np.abs(p1 - p2)


# A pressure computed in double precision is a difference of O(rho) terms: the kernels' association terms carry ~1e-13 of
# their size in rounding (measured against the oracle's long-double evaluation on the synthetic batches)
P_ROUND = 1e-13


def mix_pressure_noise(orc, params, kij, T, rho):
    """Rounding of a pressure in double precision at partial densities rho: P_ROUND sum(rho) plus the measured
    |p(double) - p(long double)| of the oracle (a dense associating phase: up to ~1e-9 rho from the site-fraction iteration --
    far above a pressure of 1e-13)."""
    rho = np.asarray(rho, dtype=np.float64)
    _, p, _, _ = orc.mix_derivatives(params, kij, T, rho, robust=True)
    _, pl, _, _ = orc.mix_derivatives_exact(params, kij, T, rho)
    return np.abs(p - pl) + P_ROUND * rho.sum(axis=1)


def gc_pressure_noise(orc, enc, phi, T, rho):
    """gc rows (no long-double evaluation): P_ROUND sum(rho) plus |p(safeguarded) - p(literal association iteration)|"""
    rho = np.asarray(rho, dtype=np.float64)
    _, p, _, _ = orc.gc_derivatives(enc, phi, T, rho, robust=True)
    _, pl, _, _ = orc.gc_derivatives(enc, phi, T, rho, robust=False)
    return np.abs(p - pl) + P_ROUND * rho.sum(axis=1)
