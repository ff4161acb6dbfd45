"""The saturation-line grid shared by tests/test_saturation_grid.py (CPU) and tests/test_saturation_line_gpu.py (GPU).

Parameter rows of all four classes (critical_referee.sample) are placed on their own saturation line by the TRUE reduced
temperature theta = T / T_c, with T_c, p_c and rho_c from critical_referee.oracle_scan (independent of every VLE solver):
every row at every theta of SUB (the oracle solves all of them) and of SUPER (no vapour-liquid equilibrium exists).

Two row orders: theta-major (row k * n_rows + i is parameter row i at THETA[k]: whole waves sit at one theta) and
`interleave` (a seeded permutation: a wave mixes theta from 0.45 to 1.03 and all four classes).

`reference` holds what the oracle alone says on the grid -- the long-double solution of every property, and per theta the
conditioning measures the GPU bars are built from: the maximum over the rows of |oracle fp64 (prec=0) - oracle long double
(prec=1)|, relative to the long-double value for densities and pressures and relative to the row's largest gradient
component for gradients.  Nothing in this file touches the GPU.
"""
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import critical_referee as cr  # noqa: E402

SUB = (0.45, 0.6, 0.8, 0.9, 0.95, 0.98, 0.99, 0.995, 0.999, 0.9995, 0.9999)
SUPER = (1.0001, 1.001, 1.01, 1.03)
THETA = SUB + SUPER
N_ROWS, SEED = 800, 21
ORDER_SEED = 5
PREFIXES = (1, 63, 64, 65, 257)
# the two liquid_density cases: p = P_SAT_FACTOR p_sat(theta) (sub-critical rows) and p = P_C_FACTOR p_c (every row)
P_SAT_FACTOR, P_C_FACTOR = 1.05, 2.0
PROPS = ("vapor_pressure", "liquid_density", "equilibrium_liquid_density")

Grid = namedtuple("Grid", "P T theta Tc pc rhoc rhoc_red row")
_CACHE = {}


def _oracle():
    from oracle import pyoracle

    pyoracle.build()
    return pyoracle


def grid(n_rows=N_ROWS, seed=SEED, orc=None):
    """-> Grid(P [n k, 8], T [K], theta, T_c [K], p_c [Pa], rho_c [kmol/m3], rho_c [A^-3], parameter-row index), each of
    n_rows * len(THETA) rows in theta-major order."""
    key = ("grid", n_rows, seed)
    if key not in _CACHE:
        orc = orc or _oracle()
        P0 = cr.sample(n_rows, seed=seed)
        Tc, pc, rc, rr = cr.oracle_scan(orc, P0)
        k = len(THETA)
        th = np.repeat(np.asarray(THETA), n_rows)
        tile = lambda x: np.tile(x, k)
        _CACHE[key] = Grid(np.ascontiguousarray(np.tile(P0, (k, 1))), th * tile(Tc), th, tile(Tc), tile(pc), tile(rc), tile(rr),
                           tile(np.arange(n_rows)))
    return _CACHE[key]


def interleave(n, seed=ORDER_SEED):
    """Seeded permutation `perm`: interleaved row j is theta-major row perm[j]."""
    return np.random.default_rng(seed).permutation(n)


def classes(P):
    """0 non-polar, 1 polar, 2 associating, 3 polar + associating."""
    return (P[:, 3] != 0).astype(np.int64) + 2 * (P[:, 4] != 0).astype(np.int64)


CLASS_NAMES = ("non-polar", "polar", "associating", "polar+assoc")


def theta_slices(g):
    """[(theta, slice of the theta-major rows)]"""
    n = len(g.T) // len(THETA)
    return [(th, slice(k * n, (k + 1) * n)) for k, th in enumerate(THETA)]


def sub_mask(g):
    return g.theta < 1.0


def liquid_pressures(g, p_sat, case):
    """Specified pressure [Pa] of the liquid_density case 'psat' (1.05 p_sat on the sub-critical rows; the super-critical
    rows, which have no p_sat, take 1.05 p_c and are only wave mates) or 'pc' (2 p_c on every row)."""
    if case == "pc":
        return P_C_FACTOR * g.pc
    return np.where(sub_mask(g), P_SAT_FACTOR * p_sat, P_SAT_FACTOR * g.pc)


def _rel(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(a - b) / np.abs(b)


def _grad_rel(a, b):
    return np.abs(a - b).max(axis=1) / np.abs(b).max(axis=1)


def _per_theta(g, err, ok):
    """max over the rows with ok of err, per theta (nan where no row is ok)."""
    out = {}
    for th, sl in theta_slices(g):
        e = err[sl][ok[sl]]
        out[th] = float(e.max()) if len(e) else float("nan")
    return out


def reference(n_rows=N_ROWS, seed=SEED, orc=None):
    """Everything the oracle says on the grid (theta-major), as a dict:
      'ld', 'f64': per precision a dict of p_sat [Pa], st_p, rho_v, rho_l [A^-3], st_vle, rho_eq [kmol/m3], st_eq,
                   rho_psat / rho_pc [kmol/m3], root_psat / root_pc [A^-3], st_psat / st_pc (True = failed);
      'p_psat', 'p_pc': the specified pressures of the two liquid_density cases;
      'grad': per property the exact gradient [n,10] at the long-double root ('liquid_density_psat', '..._pc');
      'cond': per quantity {theta: max |fp64 - long double|} (see the module docstring); for the gradients the change of
              the EXACT gradient between the oracle's long-double and its fp64 root."""
    key = ("ref", n_rows, seed)
    if key in _CACHE:
        return _CACHE[key]
    orc = orc or _oracle()
    g = grid(n_rows, seed, orc)
    out = {}
    for name, prec in (("ld", 1), ("f64", 0)):
        r = {}
        r["p_sat"], r["st_p"] = orc.pure_vapor_pressure(g.P, g.T, prec=prec)
        r["rho_v"], r["rho_l"], r["st_vle"], _, _ = orc.pure_vle(g.P, g.T, prec=prec)
        r["rho_eq"], r["st_eq"] = orc.pure_equilibrium_liquid_density(g.P, g.T, prec=prec)
        out[name] = r
    ld, f64 = out["ld"], out["f64"]
    for case in ("psat", "pc"):
        p = liquid_pressures(g, ld["p_sat"], case)
        out["p_" + case] = p
        for r, prec in ((ld, 1), (f64, 0)):
            r["rho_" + case], r["st_" + case] = orc.pure_liquid_density(g.P, g.T, p, prec=prec)
            r["root_" + case], _ = orc.pure_liquid_density_root(g.P, g.T, p, prec=prec)
    ok = ~ld["st_vle"] & ~f64["st_vle"]
    cond = {"p_sat": _per_theta(g, _rel(f64["p_sat"], ld["p_sat"]), ~ld["st_p"] & ~f64["st_p"]),
            "rho_v": _per_theta(g, _rel(f64["rho_v"], ld["rho_v"]), ok),
            "rho_l": _per_theta(g, _rel(f64["rho_l"], ld["rho_l"]), ok),
            "rho_eq": _per_theta(g, _rel(f64["rho_eq"], ld["rho_eq"]), ~ld["st_eq"] & ~f64["st_eq"])}
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = (ld["rho_l"] - ld["rho_v"]) / (ld["rho_l"] + ld["rho_v"])
    # the MINIMUM over the rows: the vapour-liquid gap is what divides the term the liquid-density Jacobians drop
    cond["gap"] = {th: -v for th, v in _per_theta(g, -gap, ok).items()}
    grad = {}
    safe = lambda x, good, f=2.0: np.where(good, x, f * g.rhoc_red)  # placeholder densities on rows that are not compared
    for prop in ("vapor_pressure", "equilibrium_liquid_density"):
        _, grad[prop] = orc.pure_property_grad(prop, g.P, g.T, None, safe(ld["rho_v"], ok, 0.5),
                                               safe(ld["rho_l"], ok), exact=True)
        _, at64 = orc.pure_property_grad(prop, g.P, g.T, None, safe(f64["rho_v"], ok, 0.5),
                                         safe(f64["rho_l"], ok), exact=True)
        cond["grad_" + prop] = _per_theta(g, _grad_rel(at64, grad[prop]), ok)
    for case in ("psat", "pc"):
        okc = ~ld["st_" + case] & ~f64["st_" + case]
        cond["rho_" + case] = _per_theta(g, _rel(f64["rho_" + case], ld["rho_" + case]), okc)
        _, grad["liquid_density_" + case] = orc.pure_property_grad("liquid_density", g.P, g.T, out["p_" + case], None,
                                                                   safe(ld["root_" + case], okc), exact=True)
        _, at64 = orc.pure_property_grad("liquid_density", g.P, g.T, out["p_" + case], None, safe(f64["root_" + case], okc),
                                         exact=True)
        cond["grad_liquid_density_" + case] = _per_theta(g, _grad_rel(at64, grad["liquid_density_" + case]), okc)
    out["grad"], out["cond"] = grad, cond
    _CACHE[key] = out
    return out


def bar(cond, theta, floor=1e-10, factor=10.0):
    """The GPU bar of an ill-conditioned quantity at one theta: max(floor, factor x the oracle's own fp64-vs-long-double
    discrepancy there).  The factor allows for a different but equally valid fp64 evaluation order."""
    c = cond[theta]
    return max(floor, factor * c) if np.isfinite(c) else floor


if __name__ == "__main__":
    import time

    t0 = time.time()
    g = grid()
    ref = reference()
    print("rows %d, oracle work %.1f s" % (len(g.T), time.time() - t0))
    keys = [k for k in ref["cond"]]
    print("theta    " + " ".join("%12s" % k[-12:] for k in keys))
    for th in THETA:
        print("%-8g " % th + " ".join("%12.2e" % ref["cond"][k][th] for k in keys))
    for th, sl in theta_slices(g):
        print("%-8g failed ld/f64: vle %d/%d p %d/%d eq %d/%d rho(1.05 psat) %d/%d rho(2 pc) %d/%d" % (
            th, ref["ld"]["st_vle"][sl].sum(), ref["f64"]["st_vle"][sl].sum(), ref["ld"]["st_p"][sl].sum(),
            ref["f64"]["st_p"][sl].sum(), ref["ld"]["st_eq"][sl].sum(), ref["f64"]["st_eq"][sl].sum(),
            ref["ld"]["st_psat"][sl].sum(), ref["f64"]["st_psat"][sl].sum(), ref["ld"]["st_pc"][sl].sum(),
            ref["f64"]["st_pc"][sl].sum()))
