"""Referee for the gradient of the incipient-phase composition of a gc bubble / dew point (test infrastructure, numpy only).

y = mole fraction of component 1 in the incipient phase (vapour for bubble, liquid for dew) of the rho4 that
oracle.pyoracle.gc_bubble_dew(..., prec=1) returns (long-double solve).  The oracle has no exact dy/dtheta, so the referee is
the construction of tests/tools/mix_incipient_referee.py: Richardson-extrapolated central differences of that solve,
    D(h) = [f(theta_k (1 + h)) - f(theta_k (1 - h))] / (2 h theta_k),     R = (4 D(h) - D(2 h)) / 3     (O(h^4)),
every displaced solve started from the base pressure, y differenced through the SMALLER of the two mole fractions.

Row set: gc_point_rows.solved (720 rows, all converged, both problems).  Directions:
  per row   phi_0, phi_1, T                                                            -> row  [m,3]
  k_ab      the four binary segment records, each as a symmetric pair, on the rows that hold both segments -> kab [m,4]
  table     every entry oracle.gc_bubble_dew_vjp_exact reports (segment used by a row, parameter != 0, which leaves out
            epsilon_k = 0 of '>C<'), on the rows that use the segment                  -> seg  [m,S,8]
k_ab and table derivatives are per-row arrays first (0 where the row does not hold the segments) and are summed under weights
afterwards: one set of displaced solves serves 'all' and every class group of gc_point_rows.groups.

The same machinery on f = p gives blocks that oracle.gc_bubble_dew_vjp_exact measures: e per group, in the measures the GPU
test applies -- gc_point_rows.row_error (phi, T per row), kab_error (records, relative to the largest) and seg_error (per
column, relative to the column's largest entry).  Bars for y: max(10 e, FLOOR) with FLOOR = 1e-8 in each of these measures
(the floor of tests/tools/mix_incipient_referee.py; for the table it applies in seg_error's column scale); the factor 10 is
the margin the mixture test gives for the difference in conditioning between p and y.

A row is dropped in advance, by the oracle alone, when a displaced solve fails, when one jumps (|dy| or |d ln p| > JUMP), or
when its own h^2 estimate exceeds FLOOR: est = |R - D(h)| in the measure of the block (phi and T as row_error; k_ab and table
entries together as logarithmic derivatives theta_k dy/dtheta_k relative to the row's largest).  Dropped rows carry weight 0
in every sum.  At most CAP of a model class may be dropped; the committed H meets that.

Measured on the oracle alone (tests/test_gc_incipient_referee.py prints them), H = 3e-6: see that file's docstring.
"""
import numpy as np

import gc_point_rows as gp
from gc_temperature_referee import sub_enc

H = 3e-6
JUMP = 1e-2
FLOOR = 1e-8
CAP = 0.10
_CACHE = {}


def molefrac(rho4, dew, component=0):
    inc = rho4[:, 2:4] if dew else rho4[:, 0:2]
    return inc[:, component] / (inc[:, 0] + inc[:, 1])


class Block:
    """Richardson (R) and plain (D) differences of p and y in a set of directions, and the rows a displaced solve spoilt"""

    def __init__(self, m, shape):
        self.Rp, self.Dp, self.Ry, self.Dy = (np.zeros((m,) + shape) for _ in range(4))


def _difference(orc, r, dew, base, rows, theta0, make, h):
    """One direction on the rows `rows`: make(factor) -> (enc, phi, T) of those rows displaced to theta0 * factor.
    -> (Rp, Dp, Ry, Dy [len(rows)], bad [len(rows)])"""
    p_base, y_base = base
    f = {}
    bad = np.zeros(len(rows), dtype=bool)
    for s in (-2, -1, 1, 2):
        enc, phi, T = make(1.0 + s * h)
        p, rho4, st = orc.gc_bubble_dew(enc, phi, T, r["x"][rows], p_base[rows], dew, prec=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            y = molefrac(rho4, dew)
            jump = ~(np.abs(y - y_base[rows]) < JUMP) | ~(np.abs(np.log(p / p_base[rows])) < JUMP)
            y = np.where(y_base[rows] <= 0.5, y, -molefrac(rho4, dew, 1))
        bad |= st | jump
        f[s] = (p, y)
    step = h * theta0
    out = []
    for j in range(2):
        d1 = (f[1][j] - f[-1][j]) / (2.0 * step)
        d2 = (f[2][j] - f[-2][j]) / (4.0 * step)
        out += [(4.0 * d1 - d2) / 3.0, d1]
    return (*out, bad)


def richardson(orc, r, dew, h=None):
    """All directions of the row set r (gc_point_rows.solved) -> dict(row, kab, seg: Block; bad [m]; reported [S,8] bool;
    p, y [m] of the base state)"""
    h = H if h is None else h
    m, enc = r["m"], r["enc"]
    all_rows = np.arange(m)
    p_base, rho4_b, st = orc.gc_bubble_dew(enc, r["phi"], r["T"], r["x"], np.full(m, 1e5), dew, prec=1)
    assert not st.any()
    y_base = molefrac(r["rho4"], dew)
    base = (p_base, y_base)
    bad = np.zeros(m, dtype=bool)
    S = enc["S"]
    row, kab, seg = Block(m, (3,)), Block(m, (len(r["kab_list"]),)), Block(m, (S, 8))

    def put(block, rows, index, res):
        for name, v in zip(("Rp", "Dp", "Ry", "Dy"), res[:4]):
            getattr(block, name)[(rows,) + index] = v
        bad[rows[res[4]]] = True

    for c in range(2):
        def make(fac, c=c):
            phi = r["phi"].copy()
            phi[:, c] *= fac
            return enc, phi, r["T"]
        put(row, all_rows, (c,), _difference(orc, r, dew, base, all_rows, r["phi"][:, c], make, h))
    put(row, all_rows, (2,), _difference(orc, r, dew, base, all_rows, r["T"], lambda fac: (enc, r["phi"], r["T"] * fac), h))

    used = enc["counts"].sum(axis=1) > 0  # [m,S]
    ident = enc["ident"]
    for k, (s1, s2, _) in enumerate(r["kab_list"]):
        a, b = ident.index(s1), ident.index(s2)
        rows = np.nonzero(used[:, a] & used[:, b])[0]
        if len(rows) == 0 or enc["kab"][a, b] == 0.0:
            continue
        sub = sub_enc(enc, rows)

        def make(fac, a=a, b=b, sub=sub, rows=rows):
            kk = enc["kab"].copy()
            kk[a, b] *= fac
            kk[b, a] = kk[a, b]
            return dict(sub, kab=kk), r["phi"][rows], r["T"][rows]
        put(kab, rows, (k,), _difference(orc, r, dew, base, rows, enc["kab"][a, b], make, h))

    reported = used.any(axis=0)[:, None] & (enc["seg"] != 0.0)
    for a in range(S):
        rows = np.nonzero(used[:, a])[0]
        if len(rows) == 0:
            continue
        sub = sub_enc(enc, rows)
        for k in range(8):
            if not reported[a, k]:
                continue

            def make(fac, a=a, k=k, sub=sub, rows=rows):
                sg = enc["seg"].copy()
                sg[a, k] *= fac
                return dict(sub, seg=sg), r["phi"][rows], r["T"][rows]
            put(seg, rows, (a, k), _difference(orc, r, dew, base, rows, enc["seg"][a, k], make, h))
    return {"row": row, "kab": kab, "seg": seg, "bad": bad, "reported": reported, "p": p_base, "y": y_base}


def estimates(r, d):
    """{phi, T, tab: [m]} the rows' own h^2 estimates |R - D(h)| of the y blocks: phi and T in the measure of
    gc_point_rows.row_error, the k_ab records and table entries together as logarithmic derivatives relative to the row's
    largest"""
    est = gp.row_error(d["row"].Dy, d["row"].Ry)
    enc = r["enc"]
    ident = enc["ident"]
    th_k = np.array([enc["kab"][ident.index(k[0]), ident.index(k[1])] for k in r["kab_list"]])
    m = r["m"]
    R = np.concatenate((d["kab"].Ry * th_k, (d["seg"].Ry * enc["seg"]).reshape(m, -1)), axis=1)
    D = np.concatenate((d["kab"].Dy * th_k, (d["seg"].Dy * enc["seg"]).reshape(m, -1)), axis=1)
    den = np.abs(R).max(axis=1)
    est["tab"] = np.abs(R - D).max(axis=1) / np.where(den == 0.0, 1.0, den)
    return est


def kab_matrix(r, per_row, w):
    """[S,S] symmetric: the records' weighted sums of a per-row block [m,4], stored at both places like the oracle's grad_kab"""
    ident = r["enc"]["ident"]
    out = np.zeros((len(ident), len(ident)))
    for k, (s1, s2, _) in enumerate(r["kab_list"]):
        a, b = ident.index(s1), ident.index(s2)
        out[a, b] = out[b, a] = float(w[w != 0.0] @ per_row[w != 0.0, k])  # (a dropped row's differences may be NaN)
    return out


def seg_sum(per_row, w):
    """[S,8]: weighted sum of a per-row table block [m,S,8]"""
    return np.tensordot(w[w != 0.0], per_row[w != 0.0], axes=(0, 0))


def quotient(Jp, Jy):
    """blocks [n,k] w.r.t. (.., T) at fixed T, T last -> dy/d(.., p_spec) along p(theta, T) = p_spec"""
    dy_dp = Jy[:, -1:] / Jp[:, -1:]
    return np.concatenate((Jy[:, :-1] - dy_dp * Jp[:, :-1], dy_dp), axis=1)


class Referee:
    pass


def referee(orc, dew):
    """The referee of one problem, cached per process: the Richardson blocks (d), the kept rows (keep), per group of
    gc_point_rows.groups the weights with the dropped rows at 0 (w), the referee's own error e (row: phi, T; kab; seg [8]) from
    the p blocks against the oracle's exact gradient, and the bars of the y blocks."""
    if dew in _CACHE:
        return _CACHE[dew]
    r = gp.solved(orc, dew)
    c = Referee()
    c.rows, c.d = r, richardson(orc, r, dew)
    c.est = estimates(r, c.d)
    c.keep = ~c.d["bad"] & (c.est["phi"] <= FLOOR) & (c.est["T"] <= FLOOR) & (c.est["tab"] <= FLOOR)
    c.y = c.d["y"]
    c.dropped_share = {int(k): float(np.mean(~c.keep[r["cls"] == k])) for k in np.unique(r["cls"])}
    c.groups = {}
    exact_all = gp.referee(orc, dew) if c.keep.all() else None
    for name, w0 in gp.groups(r).items():
        w = w0 * c.keep
        g = Referee()
        g.w = w
        if exact_all is not None:
            ex = exact_all[name]
            grow, gkab, gseg = ex["grad_row"], ex["grad_kab"], ex["grad_seg"]
        else:
            _, grow, gkab, gseg, _ = orc.gc_bubble_dew_vjp_exact(r["enc"], r["phi"], r["T"], r["rho4"], dew, w)
        on = w != 0.0
        er = gp.row_error(c.d["row"].Rp[on], grow[on])
        g.e_row = {k: float(v.max()) for k, v in er.items()}
        want_rec = gp.kab_records(r, gkab)
        g.kab_p = kab_matrix(r, c.d["kab"].Rp, w)
        g.e_kab = gp.kab_error(r, g.kab_p, gkab) if np.any(want_rec != 0.0) else 0.0
        g.seg_p = seg_sum(c.d["seg"].Rp, w)
        g.e_seg, _ = gp.seg_error(r, g.seg_p, gseg, mask_rows=on)
        g.kab_y = kab_matrix(r, c.d["kab"].Ry, w)
        g.seg_y = seg_sum(c.d["seg"].Ry, w)
        g.bar_row = {k: max(10.0 * v, FLOOR) for k, v in g.e_row.items()}
        g.bar_kab = max(10.0 * g.e_kab, FLOOR)
        g.bar_seg = np.maximum(10.0 * np.nan_to_num(g.e_seg), FLOOR)
        c.groups[name] = g
    _CACHE[dew] = c
    return c
