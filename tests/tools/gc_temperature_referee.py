"""Referee and input set for GcPcSaftMix.bubble_temperature / dew_temperature (test infrastructure, numpy only).

Referee: the T with p_oracle(T, z) = p_spec by the bracketed secant / bisection of mix_temperature_referee.solve_temperature
(on f = ln p - ln p_spec in x = 1/T), over oracle.pyoracle.gc_bubble_dew in its most precise mode (prec=1: long double).  Its
gradient is the implicit-function quotient of the oracle's exact pressure gradient at the solved state
(oracle.gc_bubble_dew_vjp_exact): per row dT/dphi = -grad_row[:, :2] / grad_row[:, 2], dT/dp_spec = 1 / grad_row[:, 2]; the
k_ab and segment-table sums are the oracle's own weighted sums under the weights w = -g / (dp/dT) for an upstream gradient g.

Input set (the GPU test uses the same): the rows of synthetic.gc_batch(N_ROWS, gc_point_rows.table(), SEED) at
T_grid = s T_batch for the factors FACTORS (T_batch is 0.6 of the lower critical-temperature estimate, so all stay
sub-critical), both problems, p_spec = the oracle's pressure at T_grid: the exact answer is T_grid.  A row is kept when the
oracle solves it at T_grid with dp/dT > 0 and at 0.93 and 1.07 T_grid (the displaced starts must be meaningful).  At most CAP
of the rows of any (class, factor, problem) cell may be dropped; the committed SEED and FACTORS meet that
(tests/test_gc_temperature_referee.py).  Classes: gc_point_rows.class_key.
"""
import numpy as np

import gc_point_rows
import mix_temperature_referee as mixref

N_ROWS, SEED = 384, 2043
FACTORS = (0.85, 1.0, 1.2)
STARTS = (1.0, 0.93, 1.07)  # first iterates, as factors of T_grid
CAP = 0.10
N_KEYS = 8  # class keys of gc_point_rows.class_key
DROPPED = (5, 400, 901)  # rows the gradient test gives a bad p_spec: they carry no weight in the referee's sums


class Inputs:
    pass


def sub_enc(enc, idx):
    """the dense encoding restricted to the rows idx"""
    return dict(enc, counts=np.ascontiguousarray(enc["counts"][idx]), bonds=np.ascontiguousarray(enc["bonds"][idx]))


class _GcRows:
    """Lets mix_temperature_referee.solve_temperature drive the gc oracle: the `parameters` it slices are row indices."""

    def __init__(self, orc, enc, phi):
        self.orc, self.enc, self.phi = orc, enc, phi

    def mix_bubble_dew(self, rows, _rows, T, z, p_init, dew, prec=1):
        return self.orc.gc_bubble_dew(sub_enc(self.enc, rows), self.phi[rows], T, z, p_init, dew, prec=prec)


def solve_temperature(orc, c, rows, p_spec, T0, dew):
    """-> T [m] (NaN where the referee fails), p [m], rho4 [m,4] for the rows `rows` of the input set c"""
    rows = np.asarray(rows)
    return mixref.solve_temperature(_GcRows(orc, c.enc, c.phi), rows, rows, c.z[rows], p_spec, T0, dew)


def quotient(grad_row):
    """[n,3] dp/d(phi_0, phi_1, T) -> [n,3] dT/d(phi_0, phi_1, p_spec)"""
    inv = 1.0 / grad_row[:, 2:3]
    return np.concatenate((-grad_row[:, :2] * inv, inv), axis=1)


_CACHE = {}


def inputs(orc, dew):
    """The input set of one problem: 3 x 384 rows, factor-major.  Cached per process, arrays read-only."""
    if dew in _CACHE:
        return _CACHE[dew]
    from feos_torch_amd.synthetic import gc_batch

    b = gc_batch(N_ROWS, gc_point_rows.table(), seed=SEED)
    e1 = orc.gc_encode(gc_point_rows.table(), b["segment_lists"], b["bond_lists"], b["kab_list"])
    c = Inputs()
    nf = len(FACTORS)
    c.n = n = nf * N_ROWS
    c.segment_lists, c.bond_lists, c.kab_list = b["segment_lists"] * nf, b["bond_lists"] * nf, b["kab_list"]
    c.enc = dict(e1, counts=np.tile(e1["counts"], (nf, 1, 1)), bonds=np.tile(e1["bonds"], (nf, 1, 1, 1)))
    c.phi, c.z = np.tile(b["phi"], (nf, 1)), np.tile(b["x"], nf)
    c.T = np.concatenate([s * b["T"] for s in FACTORS])
    c.cls = np.tile(gc_point_rows.class_key(e1["seg"], e1["counts"]), nf)
    c.factor = np.repeat(np.arange(nf), N_ROWS)
    c.cell = c.factor * N_KEYS + c.cls
    c.cells = np.unique(c.cell)
    p, rho4, st = orc.gc_bubble_dew(c.enc, c.phi, c.T, c.z, np.tile(b["p_init"], nf), dew, prec=1)
    ok = ~st & np.isfinite(p) & (p > 0)
    c.p_spec = np.where(ok, p, 1e5)  # rows the oracle does not solve stay in the batch as wave mates
    c.rho4 = np.where(ok[:, None], rho4, np.nan)
    safe = np.where(ok[:, None], rho4, np.array([1e-6, 1e-6, 5e-3, 5e-3]))
    w = ok.astype(np.float64)  # a row of weight 0 is skipped
    c.grad_row = orc.gc_bubble_dew_vjp_exact(c.enc, c.phi, c.T, safe, dew, w, segments=False)[1]
    c.grad_row64 = orc.gc_bubble_dew_vjp_exact(c.enc, c.phi, c.T, safe, dew, w, prec=0, segments=False)[1]
    with np.errstate(invalid="ignore", divide="ignore"):
        c.dlnp_dlnT = c.grad_row[:, 2] * c.T / c.p_spec
    ok &= np.isfinite(c.dlnp_dlnT) & (c.grad_row[:, 2] > 0)
    # the displaced starts: the oracle must have an equilibrium there too; the solutions also give d ln rho / d ln p along the line
    c.side = {}
    for s in STARTS[1:]:
        ps, rs, sts = orc.gc_bubble_dew(c.enc, c.phi, s * c.T, c.z, c.p_spec, dew, prec=1)
        ok &= ~sts & np.isfinite(ps) & (ps > 0)
        c.side[s] = (ps, rs)
    c.keep = ok
    (p_a, r_a), (p_b, r_b) = c.side[STARTS[1]], c.side[STARTS[2]]
    with np.errstate(invalid="ignore", divide="ignore"):
        c.dlnrho_dlnp = np.abs(np.log(r_b / r_a)).max(axis=1) / np.abs(np.log(p_b / p_a))
    c.dropped_share = {int(k): float(np.mean(~c.keep[c.cell == k])) for k in c.cells}
    c.safe_rho4 = safe
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CACHE[dew] = c
    return c


def weighted(orc, c, dew):
    """The referee of the gradient test, computed once: a seeded upstream gradient g ~ U(0.5, 1.5) of T on the kept rows (0
    elsewhere and on the rows DROPPED, which the test makes fail), the pressure weights w = -g / (dp/dT), and the oracle's
    sums under w -- exact k_ab [S,S] and segment table [S,8] with its self error [8], and the k_ab sum once more in fp64
    (kab64) for the bar."""
    key = ("weighted", dew)
    if key not in _CACHE:
        g = np.where(c.keep, np.random.default_rng(SEED + 1 + int(bool(dew))).uniform(0.5, 1.5, c.n), 0.0)
        g[list(DROPPED)] = 0.0
        with np.errstate(invalid="ignore", divide="ignore"):
            w = np.where(c.keep, -g / c.grad_row[:, 2], 0.0)
        _, _, gkab, gseg, err = orc.gc_bubble_dew_vjp_exact(c.enc, c.phi, c.T, c.safe_rho4, dew, w)
        kab64 = orc.gc_bubble_dew_vjp_exact(c.enc, c.phi, c.T, c.safe_rho4, dew, w, prec=0, segments=False)[2]
        out = {"g": g, "w": w, "grad_kab": gkab, "grad_seg": gseg, "seg_self_error": err, "kab64": kab64}
        for v in out.values():
            v.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def per_cell_max(c, values, mask):
    """[n]: for every row the largest of values[mask] over the row's (class, factor) cell (0 where the cell has none)"""
    out = np.zeros(c.n)
    for k in c.cells:
        m = (c.cell == k) & mask
        if m.any():
            out[c.cell == k] = np.nanmax(values[m])
    return out


def interleave(n):
    """a fixed permutation that mixes the factor blocks: position -> row"""
    return np.arange(n).reshape(len(FACTORS), -1).T.ravel()
