"""GPU: incipient-phase composition of GcPcSaftMix.bubble_point / dew_point (incipient_molefracs=True) and of the temperature
solve behind bubble_temperature / dew_temperature (GcPcSaftMix._point: the two public temperature methods keep their pinned
parameter lists, see _call) with its two kernels,

  pcs_gc_point_jacobian (k_gc_point_jacobian)                          jac_p, jac_y [n,7], agg [n,6]
  pcs_gc_point_segment_gradient (k_gc_segment_gradient<2, 192>)        grad_seg [S,8] += sum_i (g_p dp_i + g_y dy_i) / d table

on the row set of tests/tools/gc_point_rows.py (720 rows, classes 0, 1, 2, 3, 5, 6) against the Richardson referee of
tests/tools/gc_incipient_referee.py, at the referee's bars max(10 e, 1e-8) (tests/test_gc_incipient_referee.py: e <= 7.3e-11 for
phi and T per row, 2.3e-9 for the k_ab records, 2.9e-10 for the table columns).  The temperature calls' values use the input set
of tests/tools/gc_temperature_referee.py.

Value bars, as tests/test_mix_incipient_gpu.py forms them: max(1e-10, max(1e-10, 10 e_p) x max(1, conditioning)) per cell, e_p =
the EXISTING pressure kernel against the oracle in that cell; conditioning = |d ln y / d ln p| along T from the referee's own
blocks (pressure calls, cell = model class) resp. the temperature set's d ln rho / d ln p (temperature calls).

SPREAD: run-to-run spread of the fp64 atomics of the EXISTING pcs_gc_segment_gradient (two identical calls on the 720 rows,
largest difference relative to the column's largest entry), measured on an MI355X: see SPREAD below.  Linearity and the
gout_y = None comparison are allowed ten times that.

Measured on an MI355X: see the tests' docstrings.  The whole module takes 13 s.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import gc_incipient_referee as ref  # noqa: E402
import gc_point_rows as gp  # noqa: E402
import gc_temperature_referee as tref  # noqa: E402

pytestmark = pytest.mark.gpu

f64 = torch.float64
PROBLEMS = (False, True)
PREFIXES = (1, 63, 64, 65, 255, 256, 257, 720)
BAD = (100, 333)  # rows the autograd tests make fail
# largest |difference| of two identical pcs_gc_segment_gradient calls over the column's largest entry, MI355X, 720 rows under
# per-Pa weights, 8 pairs of calls: bubble 1.5e-14, dew 2.3e-14 (test_linearity_and_the_pressure_only_mode prints the spread
# of its own run); the smaller of the two is the constant
SPREAD = 1.5e-14
name = lambda dew: "dew" if dew else "bubble"


class Ctx:
    pass


def _d(x):
    return torch.from_numpy(np.array(x)).cuda()


def _np(x):
    return x.detach().cpu().numpy()


def _rel(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(a - b) / np.abs(b)


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64))


def _col_err(got, want):
    scale = want.abs().max(dim=0).values.clamp_min(1e-300)
    return float(((got - want).abs() / scale).max())


def _device_rows(tab, r, idx=None):
    """Device arrays of the rows idx (default: all) of a solved set on the table tab"""
    from feos_torch_amd.gc_pcsaft import build_table, encode_rows

    ident = [s for s, _ in tab]
    kab = torch.zeros((len(ident), len(ident)), dtype=f64)
    for s1, s2, k in r["kab_list"]:
        kab[ident.index(s1), ident.index(s2)] = kab[ident.index(s2), ident.index(s1)] = k
    seg = torch.tensor(np.stack([v for _, v in tab]), dtype=f64)
    idx = np.arange(r["m"]) if idx is None else np.asarray(idx)
    uniq = np.unique(idx)
    enc = encode_rows(ident, [r["segs"][k] for k in uniq], [r["bonds"][k] for k in uniq])
    return {"table": build_table(seg.cuda(), kab.cuda()), "S": len(ident), "rows": _d(enc[np.searchsorted(uniq, idx)]),
            "phi": _d(r["phi"][idx]), "T": _d(r["T"][idx]), "rho4": _d(r["rho4"][idx]), "x": _d(r["x"][idx]), "n": len(idx)}


def _pj(native, b, dew, sl=slice(None), **kw):
    return native.gc_point_jacobian(b["table"], b["S"], b["rows"][sl], b["phi"][sl], b["T"][sl], b["rho4"][sl], dew, **kw)


def _pseg(native, b, dew, sl=slice(None), **kw):
    return native.gc_point_segment_gradient(b["table"], b["S"], b["rows"][sl], b["phi"][sl], b["T"][sl], b["rho4"][sl], dew, **kw)


def _kab(b, block, g):
    """[S,S] gradient w.r.t. the symmetric k_ab pairs from a per-row block [n,7] under the weights g"""
    from feos_torch_amd.gc_pcsaft import _kab_gradient

    G = _kab_gradient(b["table"], b["S"], b["rows"], b["phi"], b["T"], g * block[:, 1], g * block[:, 4])
    return G + G.t() - torch.diag(torch.diagonal(G))


def _model(bt, grad=False, T=None, phi=None):
    """GcPcSaftMix on the whole batch bt (gc_batch fields) -> (model, segment vectors, k_ab record tensor, phi)"""
    from feos_torch_amd import GcPcSaftMix

    tab = gp.table()
    cols = [torch.tensor([v[k] for _, v in tab], dtype=f64, requires_grad=grad) for k in range(8)]
    kab = torch.tensor([k[2] for k in bt["kab_list"]], dtype=f64, requires_grad=grad)
    kl = [(k[0], k[1], kv) for k, kv in zip(bt["kab_list"], kab)]
    ph = torch.tensor(bt["phi"] if phi is None else phi, dtype=f64, requires_grad=grad)
    return GcPcSaftMix([s for s, _ in tab], tuple(cols), bt["segment_lists"], bt["bond_lists"], kl, ph), cols, kab, ph


def _call(eos, dew, temperature_call):
    """The public method; for a temperature call with the composition, GcPcSaftMix._point: the parameter lists of
    bubble_temperature / dew_temperature are pinned by tests/test_gc_temperature_referee.py and do not take the keyword."""
    if not temperature_call:
        return eos.dew_point if dew else eos.bubble_point
    public = eos.dew_temperature if dew else eos.bubble_temperature

    def call(pressure, molefracs, temperature, check_stability=False, incipient_molefracs=False):
        if not incipient_molefracs:
            return public(pressure, molefracs, temperature, check_stability)
        return eos._point(True, dew, pressure, molefracs, temperature, check_stability, True)

    return call


@pytest.fixture(scope="module")
def ctx(oracle, hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from feos_torch_amd import native

    out = {}
    for dew in PROBLEMS:
        g = Ctx()
        g.dew, g.r, g.c = dew, gp.solved(oracle, dew), ref.referee(oracle, dew)
        assert (g.r["keep"] == np.arange(gp.N)).all()  # the row set is the whole batch: model rows = set rows
        g.b = _device_rows(gp.table(), g.r)
        g.order = native.gc_class_order(g.b["table"], g.b["S"], g.b["rows"])
        g.jp, g.jy, g.agg = _pj(native, g.b, dew)
        out[dew] = g
    return out


def _value_bar(cell, e_p, cond, on):
    """max(1e-10, max(1e-10, 10 e_p) x max(1, cond)) with both factors taken per cell over the rows `on`"""
    bar = np.full(len(cell), 1e-10)
    for k in np.unique(cell):
        m = (cell == k) & on
        if m.any():
            bar[cell == k] = max(1e-10, max(1e-10, 10.0 * np.nanmax(e_p[m])) * max(1.0, np.nanmax(cond[m])))
    return bar


def _tuples(dew, temperature_call, bt, first, z, start):
    """the four tuples of one call: default, with y, with the stability flag, with both -- each on a fresh model"""
    out = []
    for kw in ({}, {"incipient_molefracs": True}, {"check_stability": True}, {"check_stability": True, "incipient_molefracs": True}):
        out.append(_call(_model(bt)[0], dew, temperature_call)(_d(first), _d(z), _d(start), **kw))
    base, with_y, base_s, with_s = out
    assert len(base) == 2 and len(with_y) == 3 and len(base_s) == 3 and len(with_s) == 4
    assert all(torch.equal(u, v) for u, v in zip(base, with_y[:2])) and all(torch.equal(u, v) for u, v in zip(base_s, with_s[:3]))
    assert torch.equal(with_s[3], with_y[2]) and torch.equal(base_s[0], base[0])
    y = with_y[2]
    assert y.dtype == f64 and y.shape == with_y[0].shape and y.device == with_y[0].device
    return with_y


@pytest.mark.parametrize("dew", PROBLEMS)
def test_values_of_the_pressure_calls(ctx, dew):
    """(p, nans[, stable]) are the default call's, element for element; y against the oracle's on the kept rows.
    Measured on an MI355X: bubble 4.8e-14 (bar <= 5.7e-10) on 720 rows, dew 1.0e-13 (bar <= 1.5e-10) on the 717 kept rows; all
    720 rows solved; y from 8.2e-13 to 1 - 3.7e-12 (bubble), 7.8e-14 to 1 - 4.8e-14 (dew)."""
    g = ctx[dew]
    r, c, bt = g.r, g.c, gp.batch()
    p, nans, y = _tuples(dew, False, bt, bt["T"], bt["x"], bt["p_init"])
    nans = _np(nans)
    k = c.keep & ~nans
    assert k.sum() >= 0.97 * c.keep.sum()
    pf, yf = np.full(r["m"], np.nan), np.full(r["m"], np.nan)
    pf[~nans], yf[~nans] = _np(p), _np(y)
    d = c.d["row"]
    with np.errstate(invalid="ignore", divide="ignore"):
        cond = np.abs(d.Ry[:, 2] / c.y) / np.abs(d.Rp[:, 2] / c.d["p"])  # |d ln y / d ln p| along T, from the oracle alone
    bar = _value_bar(r["cls"], _rel(pf, c.d["p"]), cond, k)
    err = _rel(yf, c.y)
    print("\n%-6s pressure calls: y vs oracle %.2e (bar <= %.2e) on %d rows; y in [%.3e, %.17g]" % (
        name(dew), err[k].max(), bar[k].max(), k.sum(), yf[k].min(), yf[k].max()))
    assert (err[k] <= bar[k]).all(), np.nonzero(k & ~(err <= bar))[0]
    assert (yf[k] > 0).all() and (yf[k] <= 1).all()


@pytest.mark.parametrize("dew", PROBLEMS)
def test_values_of_the_temperature_calls(oracle, hip_lib, dew):
    """Input set of tests/tools/gc_temperature_referee.py (1152 rows), start 0.93 T_grid: (T, nans[, stable]) are the default
    call's; y against the oracle's y at the referee's solved state, bar_rho of tests/test_gc_temperature_gpu.py.
    Measured on an MI355X: bubble 2.9e-12 (bar <= 5.0e-10), dew 3.9e-13 (bar <= 1.3e-10), 1152 rows each."""
    from feos_torch_amd import native

    c = tref.inputs(oracle, dew)
    bt = {"kab_list": c.kab_list, "phi": c.phi, "segment_lists": c.segment_lists, "bond_lists": c.bond_lists}
    T, nans, y = _tuples(dew, True, bt, c.p_spec, c.z, 0.93 * c.T)
    nans = _np(nans)
    eos = _model(bt)[0]
    table, rows = eos._table(), eos.rows
    sol = native.gc_bubble_dew(table, eos.S, rows, _d(c.phi), _d(c.T), _d(c.z), _d(c.p_spec), dew)
    st = _np(sol["status"])
    e = tref.per_cell_max(c, _rel(_np(sol["p"]), c.p_spec), c.keep & ~st)
    bar = np.maximum(1e-10, np.maximum(1e-10, 10.0 * e) * tref.per_cell_max(c, c.dlnrho_dlnp, c.keep))
    k = c.keep & ~nans
    assert k.sum() >= 0.97 * c.keep.sum()
    yf = np.full(c.n, np.nan)
    yf[~nans] = _np(y)
    want = ref.molefrac(np.where(c.keep[:, None], c.rho4, 1.0), dew)
    err = _rel(yf, want)
    print("\n%-6s temperature calls: y vs oracle %.2e (bar <= %.2e) on %d rows" % (name(dew), err[k].max(), bar[k].max(), k.sum()))
    assert (err[k] <= bar[k]).all(), np.nonzero(k & ~(err <= bar))[0]
    assert (yf[k] > 0).all() and (yf[k] <= 1).all()


@pytest.mark.parametrize("dew", PROBLEMS)
def test_jac_p_and_agg_have_the_bits_of_pcs_gc_jacobian(ctx, dew):
    """The pressure block does not depend on whether the composition block is asked for, nor on the entry point.
    pcs_gc_jacobian and pcs_gc_point_jacobian share one kernel template now (pcs_gc_jacobian launches <true, false>), so the
    only_p line compares a kernel with itself; what it stood for, the bits of the kernel pcs_gc_jacobian used to have, is
    held by tests/test_gc_jacobian_bits_gpu.py."""
    from feos_torch_amd import native

    g = ctx[dew]
    b = g.b
    jac, agg = native.gc_jacobian(b["table"], b["S"], b["rows"], b["phi"], b["T"], b["rho4"], dew)
    assert bool(torch.isfinite(g.jp).all()) and bool(torch.isfinite(g.jy).all())
    assert _same_bits(g.jp, jac) and _same_bits(g.agg, agg)
    only_p = _pj(native, b, dew, want_y=False)
    only_y = _pj(native, b, dew, want_p=False)
    assert only_p[1] is None and only_y[0] is None
    assert _same_bits(only_p[0], jac) and _same_bits(only_y[1], g.jy) and _same_bits(only_p[2], agg) and _same_bits(only_y[2], agg)


@pytest.mark.parametrize("dew", PROBLEMS)
def test_jac_y_per_row_against_the_referee(ctx, dew):
    """jac_y chained on the host into phi (2) and T, every kept row, gc_point_rows.row_error, bars max(10 e, 1e-8) = 1e-8.
    Measured on an MI355X: bubble phi 9.1e-11, T 2.3e-9 (720 rows); dew phi 9.9e-11, T 2.8e-9 (717 rows) -- T is of the size
    of the referee's own h^2 estimate on those rows (<= 2.7e-9)."""
    from feos_torch_amd.gc_pcsaft import _phi_gradient

    g = ctx[dew]
    c, b = g.c, g.b
    got = np.concatenate([_np(_phi_gradient(g.jy, g.agg, b["phi"])), _np(g.jy[:, 6:7])], axis=1)
    err = gp.row_error(got, c.d["row"].Ry)
    bars = c.groups["all"].bar_row
    k = c.keep
    print("\n%-6s jac_y per row: phi %.2e (bar %.2e), T %.2e (bar %.2e) on %d rows" % (
        name(dew), err["phi"][k].max(), bars["phi"], err["T"][k].max(), bars["T"], k.sum()))
    for key in ("phi", "T"):
        assert (err[key][k] <= bars[key]).all(), (key, np.nonzero(k & ~(err[key] <= bars[key]))[0], err[key][k].max())


@pytest.mark.parametrize("dew", PROBLEMS)
def test_jac_y_records_and_table_against_the_referee(ctx, dew):
    """gout_y = w 1[class], gout_p = None: the k_ab records (host chain of jac_y) and the table, group by group.
    Measured on an MI355X, worst group: bubble k_ab 6.4e-9 (induced, polar; bar 1.8e-8), table 9.2e-10 (m of cross; bar 1e-8);
    dew k_ab 2.6e-9 (self, polar; bar 2.2e-8), table 7.9e-10 (m of none); whole set: k_ab 1.8e-9 / 2.3e-9, table 3.2e-10 / 2.8e-10."""
    from feos_torch_amd import native

    g = ctx[dew]
    c, r, b = g.c, g.r, g.b
    print("\n   %s" % name(dew))
    failures = []
    for gname, q in c.groups.items():
        w = _d(q.w)
        got = _np(_pseg(native, b, dew, gout_y=w))
        assert np.isfinite(got).all()
        err, used = gp.seg_error(r, got, q.seg_y, mask_rows=q.w != 0.0)
        assert np.all(got[~used] == 0.0), gname
        want_k = gp.kab_records(r, q.kab_y)
        got_k = _np(_kab(b, g.jy, w))
        ek = gp.kab_error(r, got_k, q.kab_y) if np.any(want_k != 0.0) else 0.0
        assert np.all(gp.kab_records(r, got_k)[want_k == 0.0] == 0.0), gname
        print("      %-15s k_ab %.2e (%.2e)  table " % (gname, ek, q.bar_kab)
              + " ".join("-" if np.isnan(e) else "%.1e" % e for e in err) + "  (bar %.1e)" % q.bar_seg.max())
        if not ek <= q.bar_kab:
            failures.append((gname, "k_ab", ek, q.bar_kab))
        for k in range(8):
            if not np.isnan(err[k]) and not err[k] <= q.bar_seg[k]:
                failures.append((gname, k, float(err[k]), float(q.bar_seg[k])))
    assert not failures, failures


@pytest.mark.parametrize("dew", PROBLEMS)
def test_linearity_and_the_pressure_only_mode(ctx, dew):
    """grad(gout_p = a, gout_y = b) = grad(a, None) + grad(None, b), and grad(a, None) = pcs_gc_segment_gradient(gout = a),
    within 10 x SPREAD of the column's largest entry; with and without the class order.
    Measured on an MI355X (three runs): spread of the run 1.5e-14 ... 2.3e-14; linearity 3.6e-14 / 4.8e-14 (bubble), 2.7e-14
    (dew); pressure-only mode 7.0e-15 / 1.0e-14 (bubble), 1.3e-14 / 9.3e-15 (dew).  (The spread is not 1e-16: under per-Pa weights
    the columns are sums of terms of both signs.)"""
    from feos_torch_amd import native

    g = ctx[dew]
    b, r = g.b, g.r
    rng = np.random.default_rng(11 + int(dew))
    # weights of the size the shell hands over: per Pa for p, O(1) for y
    a, w = _d(rng.uniform(0.5, 1.5, r["m"]) / g.c.d["p"]), _d(rng.uniform(0.5, 1.5, r["m"]))
    old = lambda **kw: native.gc_segment_gradient(b["table"], b["S"], b["rows"], b["phi"], b["T"], b["rho4"], dew, gout=a, **kw)
    first = old()
    spread = max(_col_err(old(), first) for _ in range(8))
    worst = [0.0, 0.0]
    for order in (None, g.order):
        both = _pseg(native, b, dew, gout_p=a, gout_y=w, order=order)
        p_only, y_only = _pseg(native, b, dew, gout_p=a, order=order), _pseg(native, b, dew, gout_y=w, order=order)
        worst[0] = max(worst[0], _col_err(p_only + y_only, both))
        worst[1] = max(worst[1], _col_err(p_only, old(order=order)))
    print("\n%-6s spread of this run %.2e (SPREAD %.2e); linearity %.2e, pressure-only mode %.2e" % (name(dew), spread, SPREAD, *worst))
    assert worst[0] <= 10.0 * SPREAD and worst[1] <= 10.0 * SPREAD, worst


def _referee_sums(g, wp, wy, along_pressure=False, wT=None):
    """The referee's gradient of sum_i (wp_i p_i + wy_i y_i) -- or, along constant pressure, of sum_i (wT_i T_i + wy_i y_i) --
    from its Richardson blocks: (row [m,3] w.r.t. phi_0, phi_1 and T resp. p_spec, k_ab [S,S], table [S,8])"""
    c, r = g.c, g.r
    d = c.d
    row_p, row_y = d["row"].Rp, d["row"].Ry
    if along_pressure:
        inv = 1.0 / row_p[:, 2]
        total = wT + wy * row_y[:, 2]       # dL/dT at fixed theta
        with np.errstate(invalid="ignore"):
            wp = np.where(total != 0.0, -total * inv, 0.0)  # weight of the pressure's gradients
            inv = np.where(total != 0.0, inv, 0.0)
        row = np.concatenate((wp[:, None] * row_p[:, :2] + wy[:, None] * row_y[:, :2], (total * inv)[:, None]), axis=1)
    else:
        row = wp[:, None] * row_p + wy[:, None] * row_y
    kab = ref.kab_matrix(r, d["kab"].Rp, wp) + ref.kab_matrix(r, d["kab"].Ry, wy)
    seg = ref.seg_sum(d["seg"].Rp, wp) + ref.seg_sum(d["seg"].Ry, wy)
    return row, kab, seg


def _check_autograd(g, what, cols, kab, ph, given, on, want, tag):
    c, r = g.c, g.r
    q = c.groups["all"]
    row, kabm, seg = want
    got_row = np.concatenate((_np(ph.grad), _np(given.grad)[:, None]), axis=1)
    assert (got_row[~on] == 0).all(), "rows without weight or dropped rows receive exactly zero"
    err = gp.row_error(got_row[on], row[on])
    got_seg = np.stack([_np(v.grad) for v in cols], axis=1)
    es, used = gp.seg_error(r, got_seg, seg, mask_rows=on)
    assert np.all(got_seg[~used] == 0.0)
    want_k = gp.kab_records(r, kabm)
    ek = float(np.max(np.abs(_np(kab.grad) - want_k)) / np.max(np.abs(want_k)))
    print("   %-6s %-12s %-5s phi %.2e T|p %.2e k_ab %.2e table %.2e" % (
        name(g.dew), tag, what, err["phi"].max(), err["T"].max(), ek, np.nanmax(es)))
    assert err["phi"].max() <= q.bar_row["phi"] and err["T"].max() <= q.bar_row["T"], (what, err["phi"].max(), err["T"].max())
    assert ek <= q.bar_kab, (what, ek, q.bar_kab)
    assert all(np.isnan(e) or e <= bar for e, bar in zip(es, q.bar_seg)), (what, es, q.bar_seg)


@pytest.mark.parametrize("dew", PROBLEMS)
def test_autograd_of_the_pressure_calls(ctx, dew):
    """Losses on p only, y only and both (p weighted per Pa so that neither swamps the other), two rows made hopeless so that
    Compaction is in the path: gradients to the eight segment vectors, the k_ab records, phi and temperature against the
    referee's blocks under the same weights, at the referee's bars; an unused output costs nothing and raises nothing; the
    model is reduced as the default call reduces it.
    Measured on an MI355X, largest over the three losses: bubble phi 9.1e-11, T 2.3e-9, k_ab 1.9e-9, table 6.5e-10; dew
    9.9e-11, 2.8e-9, 2.1e-9, 2.4e-10."""
    g = ctx[dew]
    c, r, bt = g.c, g.r, gp.batch()
    m = r["m"]
    Tn = bt["T"].copy()
    Tn[BAD[0]], Tn[BAD[1]] = np.nan, -10.0
    on = c.keep.copy()
    on[list(BAD)] = False
    rng = np.random.default_rng(21 + int(dew))
    wp, wy = (np.where(on, rng.uniform(0.5, 1.5, m), 0.0) for _ in range(2))
    wp = wp / c.d["p"]
    print()
    for what, up, uy in (("p", True, False), ("y", False, True), ("both", True, True)):
        eos, cols, kab, ph = _model(bt, grad=True)
        T = torch.tensor(Tn, dtype=f64, requires_grad=True)
        x, p0 = torch.tensor(bt["x"], dtype=f64, requires_grad=True), torch.tensor(bt["p_init"], dtype=f64, requires_grad=True)
        p, nans, y = _call(eos, dew, False)(T, x, p0, incipient_molefracs=True)
        nans = nans.cpu().numpy()
        assert nans[list(BAD)].all() and nans.sum() == 2 and eos.rows.shape[0] == m - 2 == eos.phi.shape[0] == p.shape[0]
        ref_eos = _model(bt)[0]
        _call(ref_eos, dew, False)(torch.tensor(Tn, dtype=f64), x.detach(), p0.detach())
        assert torch.equal(ref_eos.rows, eos.rows) and torch.equal(ref_eos.phi, eos.phi.detach())
        loss = 0.0
        if up:
            loss = loss + (_d(wp[~nans]).to(p.device) * p).sum()
        if uy:
            loss = loss + (_d(wy[~nans]).to(y.device) * y).sum()
        loss.backward()
        assert x.grad is None and p0.grad is None  # mole fractions and the initial pressure receive no gradient
        want = _referee_sums(g, wp if up else 0.0 * wp, wy if uy else 0.0 * wy)
        _check_autograd(g, what, cols, kab, ph, T, on, want, "pressure")


@pytest.mark.parametrize("dew", PROBLEMS)
def test_autograd_of_the_temperature_calls(ctx, dew):
    """bubble_temperature / dew_temperature at p_spec = the oracle's pressure of the row set, start 0.97 T: losses on y only and
    on T and y; gradients to the segment vectors, k_ab, phi and PRESSURE against the referee's quotient along p = p_spec.
    Measured on an MI355X, larger of the two losses: bubble phi 1.0e-10, p_spec 2.8e-9, k_ab 1.9e-9, table 6.8e-10; dew
    1.3e-10, 2.8e-9, 2.0e-9, 2.3e-10."""
    g = ctx[dew]
    c, r, bt = g.c, g.r, gp.batch()
    m = r["m"]
    ps_np = c.d["p"].copy()
    ps_np[list(BAD)] = -1.0  # two rows fail at once
    on = c.keep.copy()
    on[list(BAD)] = False
    rng = np.random.default_rng(31 + int(dew))
    wT, wy = (np.where(on, rng.uniform(0.5, 1.5, m), 0.0) for _ in range(2))
    wT = wT / r["T"]
    print()
    for what, uT in (("y", False), ("T + y", True)):
        eos, cols, kab, ph = _model(bt, grad=True)
        ps = torch.tensor(ps_np, dtype=f64, requires_grad=True)
        x, t0 = torch.tensor(bt["x"], dtype=f64, requires_grad=True), torch.tensor(0.97 * bt["T"], dtype=f64, requires_grad=True)
        T, nans, y = _call(eos, dew, True)(ps, x, t0, incipient_molefracs=True)
        nans = nans.cpu().numpy()
        assert nans[list(BAD)].all()
        on_k = on & ~nans
        assert on_k.sum() >= 0.97 * on.sum() and eos.rows.shape[0] == int((~nans).sum())
        wTk, wyk = np.where(on_k, wT, 0.0) * float(uT), np.where(on_k, wy, 0.0)
        loss = (_d(wyk[~nans]).to(y.device) * y).sum()
        if uT:
            loss = loss + (_d(wTk[~nans]).to(T.device) * T).sum()
        loss.backward()
        assert x.grad is None and t0.grad is None  # mole fractions and the first iterate receive no gradient
        want = _referee_sums(g, None, wyk, along_pressure=True, wT=wTk)
        _check_autograd(g, what, cols, kab, ph, ps, on_k, want, "temperature")


@pytest.mark.parametrize("dew", PROBLEMS)
def test_unused_outputs(ctx, dew):
    """A loss on one output alone leaves the other's upstream gradient absent: no error, and inputs that do not reach the loss
    get None; the y-only and p-only gradients add up to the gradient of the sum (one kernel pass each) to 1e-12 of the
    column scale / of the row's entry (order of summation only, the bound of tests/test_gc_point_grad_gpu.py for the shell)."""
    g = ctx[dew]
    bt = gp.batch()
    grads = {}
    for what in ("p", "y", "both"):
        eos, cols, kab, ph = _model(bt, grad=True)
        T = torch.tensor(bt["T"], dtype=f64, requires_grad=True)
        p, nans, y = _call(eos, dew, False)(T, torch.tensor(bt["x"]), torch.tensor(bt["p_init"]), incipient_molefracs=True)
        scale = 1.0 / p.detach()
        loss = {"p": (p * scale).sum(), "y": y.sum(), "both": (p * scale).sum() + y.sum()}[what]
        out = torch.autograd.grad(loss, [*cols, T], allow_unused=True)
        assert all(v is not None for v in out)
        grads[what] = (torch.stack(out[:8], dim=1), out[8])
    assert _col_err(grads["p"][0] + grads["y"][0], grads["both"][0]) < 1e-12
    assert float(((grads["p"][1] + grads["y"][1] - grads["both"][1]).abs() / grads["both"][1].abs().clamp_min(1e-300)).max()) < 1e-12
    eos, cols, kab, ph = _model(bt, grad=True)
    p, nans, y = _call(eos, dew, False)(torch.tensor(bt["T"]), torch.tensor(bt["x"]), torch.tensor(bt["p_init"]), incipient_molefracs=True)
    out = torch.autograd.grad(y.sum(), [cols[0], kab, ph], allow_unused=True)
    assert all(v is not None and bool(torch.isfinite(v).all()) for v in out)


@pytest.mark.parametrize("dew", PROBLEMS)
def test_schedule_independence(ctx, dew):
    """jac_y (and jac_p, agg) bit-identical with and without the class order and for row prefixes around the 64-lane wave and
    the 256-row workgroup of k_gc_point_jacobian."""
    from feos_torch_amd import native

    g = ctx[dew]
    b = g.b
    jp, jy, agg = _pj(native, b, dew, order=g.order)
    assert _same_bits(jy, g.jy) and _same_bits(jp, g.jp) and _same_bits(agg, g.agg)
    for n in PREFIXES:
        jp, jy, agg = _pj(native, b, dew, slice(0, n))
        assert jy.shape == (n, 7) and _same_bits(jy, g.jy[:n]) and _same_bits(jp, g.jp[:n]) and _same_bits(agg, g.agg[:n]), n
        od = native.gc_class_order(b["table"], b["S"], b["rows"][:n])
        assert _same_bits(_pj(native, b, dew, slice(0, n), order=od)[1], g.jy[:n]), n


@pytest.mark.parametrize("dew", PROBLEMS)
def test_segment_gradient_tiles_and_padded_table(ctx, oracle, dew):
    """k_gc_segment_gradient<2, 192>: head + tail = whole at the tile edges 191 / 192 / 193 (1e-12 of the column scale, the
    bound of tests/test_gc_point_grad_gpu.py for this reduction), and the table padded to S = 32 -- the whole LDS of a CU --
    gives the full table's result on the shared segments to 1e-12 and exactly 0 on the padding.
    Measured on an MI355X: cuts 1.2e-14, padded table 3.6e-14 (bubble); 2.1e-14, 3.0e-15 (dew); jac_y on the padded table
    bit-identical."""
    from feos_torch_amd import native

    g = ctx[dew]
    b, r = g.b, g.r
    rng = np.random.default_rng(41 + int(dew))
    a, w = _d(rng.uniform(0.5, 1.5, r["m"]) / g.c.d["p"]), _d(rng.uniform(0.5, 1.5, r["m"]))
    whole = _pseg(native, b, dew, gout_p=a, gout_y=w)
    assert bool(torch.isfinite(whole).all())
    worst = 0.0
    for n in (191, 192, 193):
        head = _pseg(native, b, dew, slice(0, n), gout_p=a[:n], gout_y=w[:n])
        tail = _pseg(native, b, dew, slice(n, r["m"]), gout_p=a[n:], gout_y=w[n:])
        worst = max(worst, _col_err(head + tail, whole))
    table = gp.table()
    padded = list(table) + [(f"pad{k}", table[k % len(table)][1].copy()) for k in range(32 - len(table))]
    bp = _device_rows(padded, r)
    assert bp["S"] == 32
    gp32 = _pseg(native, bp, dew, gout_p=a, gout_y=w)
    assert bool((gp32[len(table):] == 0.0).all())
    e32 = _col_err(gp32[: len(table)], whole)
    jy32 = _pj(native, bp, dew)[1]
    ej = float(((jy32 - g.jy).abs() / g.jy.abs().clamp_min(1e-300)).max())
    print("\n%-6s cuts at 191 / 192 / 193: %.2e; table padded to S = 32: grad_seg %.2e, jac_y %.2e" % (name(dew), worst, e32, ej))
    assert worst < 1e-12 and e32 < 1e-12 and ej < 1e-12


def test_segment_gradient_past_the_persistent_grid(ctx):
    """2048 x 192 + 1 = 393 217 rows, tiled from the 720-row bubble set: the persistent grid of 682 workgroups runs its tile
    loop three times and ends on a one-row tile.  The result equals 546 x the small set's + that of its first 97 rows to 1e-11
    of the column scale (the bound of tests/test_gc_point_grad_gpu.py::test_mode0_grid_stride_wraps).  Measured on an MI355X: 1.8e-14."""
    from feos_torch_amd import native

    g = ctx[False]
    r, small = g.r, g.b
    m = r["m"]
    n = 2048 * 192 + 1
    q, rem = divmod(n, m)
    b = _device_rows(gp.table(), r, np.arange(n) % m)
    rng = np.random.default_rng(51)
    a, w = rng.uniform(0.5, 1.5, m) / g.c.d["p"], rng.uniform(0.5, 1.5, m)
    tile = lambda v: _d(np.resize(v, n))
    got = _pseg(native, b, False, gout_p=tile(a), gout_y=tile(w), order=native.gc_class_order(b["table"], b["S"], b["rows"]))
    want = q * _pseg(native, small, False, gout_p=_d(a), gout_y=_d(w)) + \
        _pseg(native, small, False, slice(0, rem), gout_p=_d(a[:rem]), gout_y=_d(w[:rem]))
    err = _col_err(got, want)
    print("\n%d rows (%d x %d + %d): grad_seg against the scaled small-set result %.2e" % (n, q, m, rem, err))
    assert bool(torch.isfinite(got).all()) and err < 1e-11, err


@pytest.mark.parametrize("dew", PROBLEMS)
def test_bad_rows_do_not_disturb_their_wave_mates(ctx, dew):
    """Failed rows of a solve (rho4 = 0) and rows at the trivial solution (incipient = specified phase: the 3x3 system of the
    model is singular there; in floating point the elimination meets a zero or a tiny pivot, so such a row is NaN or
    meaningless) in the batch: the call returns cleanly and every other row keeps its bits."""
    from feos_torch_amd import native

    g = ctx[dew]
    b = dict(g.b)
    n = b["n"]
    rho4 = b["rho4"].clone()
    zero, trivial = [0, 7, 64, 200, 383, n - 1], [1, 63, 65, 255, 256, 500]
    rho4[zero] = 0.0
    for k in trivial:
        rho4[k, 0:2] = rho4[k, 2:4]
    b["rho4"] = rho4
    other = torch.ones(n, dtype=torch.bool, device="cuda")
    other[zero + trivial] = False
    for order in (None, g.order):
        jp, jy, agg = _pj(native, b, dew, order=order)
        torch.cuda.synchronize()
        assert _same_bits(jp[other], g.jp[other]) and _same_bits(jy[other], g.jy[other]) and _same_bits(agg, g.agg)
