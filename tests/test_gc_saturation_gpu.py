"""GPU: pcs_gc_pure_vle and GcPcSaftMix.vapor_pressure / equilibrium_liquid_density against the long-double referee of
tests/tools/gc_saturation_referee.py (a fixed-grid scan of the pure line and Newton on (p, mu), independent of the kernel).

The 3,072-row set (2 components x 4 temperature factors x 384 rows, interleaved so that factors, components and classes mix
within a wave) is run once per component; a component's call is compared on the rows whose temperature was made for it, the
other half are its wave mates (some solve, some are super-critical).

Bars.  Values (p_sat, rho_V, rho_L, dp/drho at both roots): 10 x the error of the referee's fp64 twin on the same row, floor
1e-12 relative.  Gradients through the public methods: per-row columns (phi_0, phi_1, T) 1e-10 of the row's largest exact
component and the k_ab records 1e-10 of the largest record (the oracle's exact VJP has no fp64 twin, so max(1e-10, 10 x twin)
is 1e-10); segment-table columns GRAD_TOL = 1e-7 of tests/test_gc_density_gpu.py, the bar of this VJP kernel against this
referee's Richardson table differences.  Consistency with liquid_density / vapor_density at p_sat: 1e-10 / dpdrho.

Measured (MI355X, component 0 / 1): p_sat 1.2e-14 / 1.4e-14, rho_V 2.1e-14 / 1.7e-14, rho_L 6.9e-15 / 8.0e-15, dp/drho 4.5e-14 /
3.3e-14 (vapour root) and 5.9e-14 / 8.4e-14 (liquid root), at most 8 % of the bar; evaluations per solved row: median 38, at most
177.  Gradients, largest over all groups: p_sat per-row 2.4e-14 / 2.1e-14, segment table 8.8e-11 / 7.9e-11; rho_L per-row 4.3e-14 /
6.3e-14, segment table 1.5e-11 / 1.7e-11; k_ab records exactly zero on both sides (the model applies k_ab between unlike
molecules only).  Density kernels at p_sat: 4.0e-14 (liquid) / 1.2e-14 (vapour).  Full rows 6.8e-15.  The module takes 24 s, 15 s
of them the referee's input set.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import gc_saturation_referee as ref  # noqa: E402
import gc_point_rows as gp  # noqa: E402
import gc_full_rows as fr  # noqa: E402

pytestmark = pytest.mark.gpu

COMPONENTS = (0, 1)
KEYS = ("p_sat", "rho_vl", "dpdrho_vl", "status", "iters")
GRAD_TOL = 1e-7   # tests/test_gc_density_gpu.py
ROW_TOL = 1e-10
FLOOR = 1e-12
f64 = torch.float64
OUTPUT = ("p_sat", "rho_L")


class Ctx:
    pass


def _d(x):
    return torch.from_numpy(np.array(x)).cuda()


def _np(x):
    return x.detach().cpu().numpy()


def _bits(x):
    x = _np(x)
    return x.view(np.int64) if x.dtype == np.float64 else x


def _model(c, rows, grad=False, table=None):
    """GcPcSaftMix on the rows `rows` of the base set -> (model, segment vectors, k_ab record tensor, phi)"""
    from feos_torch_amd import GcPcSaftMix

    tab = gp.table() if table is None else table
    cols = [torch.tensor([v[k] for _, v in tab], dtype=f64, requires_grad=grad) for k in range(8)]
    kab = torch.tensor([k[2] for k in c.kab_list], dtype=f64, requires_grad=grad)
    kl = [(k[0], k[1], kv) for k, kv in zip(c.kab_list, kab)]
    ph = torch.tensor(c.m.phi[rows], dtype=f64, requires_grad=grad)
    eos = GcPcSaftMix([s for s, _ in tab], tuple(cols), [c.segment_lists[i] for i in rows], [c.bond_lists[i] for i in rows], kl, ph)
    return eos, cols, kab, ph


@pytest.fixture(scope="module")
def ctx(oracle, hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from feos_torch_amd import native

    c = ref.inputs(oracle)
    g = Ctx()
    g.c = c
    eos = _model(c, np.arange(ref.N_ROWS))[0]
    g.table, g.S = eos._table(), eos.S
    g.perm = ref.interleave(c.n)
    g.back = np.argsort(g.perm)
    g.rows = eos.rows[_d(c.row[g.perm])].contiguous()
    g.phi, g.T = _d(c.phi[g.perm]), _d(c.T[g.perm])
    g.order = native.gc_class_order(g.table, g.S, g.rows)
    g.r = {k: native.gc_pure_vle(g.table, g.S, g.rows, g.phi, g.T, k, order=g.order) for k in COMPONENTS}
    g.out = {k: {key: _np(g.r[k][key])[g.back] for key in KEYS} for k in COMPONENTS}  # in the referee's row order
    return g


def _run(g, comp, n=None, order=None, **changed):
    from feos_torch_amd import native

    sl = slice(0, n)
    args = {"phi": g.phi[sl], "T": g.T[sl]}
    args.update(changed)
    rows = g.rows[sl]
    od = native.gc_class_order(g.table, g.S, rows) if order is True else order
    return native.gc_pure_vle(g.table, g.S, rows, args["phi"], args["T"], comp, order=od, want=changed.get("want", KEYS))


@pytest.mark.parametrize("comp", COMPONENTS)
def test_values_against_the_referee(ctx, comp):
    c, o = ctx.c, ctx.out[comp]
    k = c.keep & (c.comp == comp)
    assert k.sum() >= 1300
    assert not o["status"][k].any(), np.nonzero(k & o["status"])[0]
    twin = ref.twin_error(c)
    got = {"p_sat": o["p_sat"], "rho_v": o["rho_vl"][:, 0], "rho_l": o["rho_vl"][:, 1], "dp_v": o["dpdrho_vl"][:, 0], "dp_l": o["dpdrho_vl"][:, 1]}
    want = {"p_sat": c.p_sat, "rho_v": c.rho_v, "rho_l": c.rho_l, "dp_v": c.dp_v, "dp_l": c.dp_l}
    fails = []
    for name in got:
        e = np.abs(got[name][k] / want[name][k] - 1.0)
        bar = np.maximum(FLOOR, 10.0 * twin[name][k])
        print("component %d, %-5s: %d rows, max relative error %.2e (twin %.2e), largest error / bar %.3f"
              % (comp, name, k.sum(), e.max(), np.nanmax(twin[name][k]), (e / bar).max()))
        if not (e <= bar).all():
            fails.append((name, float(e.max()), float((e / bar).max())))
    ev = o["iters"][~o["status"]]
    print("component %d: evaluations per solved row: median %d, max %d; %d of %d rows failed (wave mates included)"
          % (comp, np.median(ev), ev.max(), o["status"].sum(), c.n))
    assert not fails, fails
    st = o["status"]
    assert (o["iters"][~st] >= 1).all() and (o["iters"][st] == -1).all()
    assert (o["p_sat"][st] == 0.0).all() and (o["rho_vl"][st] == 0.0).all() and (o["dpdrho_vl"][st] == 0.0).all()
    # no solved row, wave mates included, carries a trivial solution or an equilibrium between two dense states
    rv, rl = o["rho_vl"][~st, 0], o["rho_vl"][~st, 1]
    assert (rv < rl * (1.0 - 1e-6)).all() and (o["p_sat"][~st] * ref.P_RED / _np(ctx.T)[ctx.back][~st] <= 1.0001 * rv).all()


@pytest.mark.parametrize("comp", COMPONENTS)
@pytest.mark.parametrize("which", (0, 1))
def test_gradients_through_the_public_methods(ctx, oracle, which, comp):
    """vapor_pressure / equilibrium_liquid_density with requires_grad on the eight segment vectors, k_ab, phi and T, under the
    referee's seeded weights: for the whole set and once per model class with the weights masked to it."""
    c = ctx.c
    wt = ref.weighted(oracle, c, which, comp)
    sel = np.nonzero(c.comp == comp)[0]
    pos = {int(r): j for j, r in enumerate(sel)}
    eos, cols, kab, ph = _model(c, c.row[sel], grad=True)
    T = torch.tensor(c.T[sel], dtype=f64, requires_grad=True)
    value, nans = (eos.vapor_pressure if which == 0 else eos.equilibrium_liquid_density)(T, component=comp)
    assert not _np(nans)[c.keep[sel]].any()
    assert not nans.any(), "the whole set solves, so the model is not reduced and value is aligned with sel"
    unit = 1.0 if which == 0 else 1.0 / ref.C_UNIT  # the referee's weights are per A^-3
    rowsd = {"enc": c.m.enc, "kab_list": c.kab_list}
    groups = {"all": np.ones(c.n, dtype=bool)}
    groups.update({gp.CLASS_NAMES[k]: c.cls == k for k in wt["groups"]})
    leaves = [*cols, kab, ph, T]
    fails, worst = [], [0.0, 0.0, 0.0]
    for gname, mask in groups.items():
        weights = np.where(mask, wt["g"], 0.0)[sel]
        for leaf in leaves:
            leaf.grad = None
        (value * _d(weights * unit).to(value.device)).sum().backward(retain_graph=True)
        row = np.concatenate((_np(ph.grad), _np(T.grad)[:, None]), axis=1)
        seg = np.stack([_np(col.grad) for col in cols], axis=1)
        got_k = _np(kab.grad)
        assert np.isfinite(row).all() and np.isfinite(seg).all() and np.isfinite(got_k).all(), gname
        if gname == "all":
            want_kab, want_seg = wt["all"]["grad_kab"], wt["all"]["grad_seg"]
            ids = np.concatenate([v["rows"] for v in wt["groups"].values()])
            want_row = np.concatenate([v["row"] for v in wt["groups"].values()])
        else:
            v = wt["groups"][[k for k in wt["groups"] if gp.CLASS_NAMES[k] == gname][0]]
            want_kab, want_seg, ids, want_row = v["grad_kab"], v["grad_seg"], v["rows"], v["row"]
        at = np.array([pos[int(r)] for r in ids])
        e_row = float((np.abs(row[at] - want_row) / np.abs(want_row).max(axis=1, keepdims=True)).max())
        off = np.ones(len(sel), dtype=bool)
        off[at] = False
        assert (row[off] == 0.0).all(), gname  # rows without weight carry no gradient
        want_k = gp.kab_records(rowsd, want_kab)
        if np.max(np.abs(want_k)) == 0.0:
            # the model applies k_ab between segments of UNLIKE molecules only (csrc/gc_model.hpp, i != j), so a pure fluid does
            # not feel it: the referee's records are exactly zero, and the public methods must hand back exact zeros too
            e_kab = 0.0 if np.all(got_k == 0.0) else np.inf
        else:
            e_kab = float(np.max(np.abs(got_k - want_k)) / np.max(np.abs(want_k)))
        sub = dict(rowsd, enc=dict(c.m.enc, counts=c.m.enc["counts"][c.row[sel]]))
        e_seg, used = gp.seg_error(sub, seg, want_seg, mask_rows=weights != 0.0)
        if not np.all(seg[~used] == 0.0):
            fails.append((gname, "segments no row uses must have zero gradient"))
        e_seg_max = float(np.nanmax(e_seg))
        print("%s, component %d, %-14s %5d rows: per-row %.2e (bar %.0e), k_ab records %.2e (bar %.0e), segment table %.2e (bar %.0e)"
              % (OUTPUT[which], comp, gname, len(ids), e_row, ROW_TOL, e_kab, ROW_TOL, e_seg_max, GRAD_TOL))
        worst = [max(a, b) for a, b in zip(worst, (e_row, e_kab, e_seg_max))]
        if not (e_row <= ROW_TOL and e_kab <= ROW_TOL and e_seg_max <= GRAD_TOL):
            fails.append((gname, e_row, e_kab, e_seg_max))
    print("%s, component %d: largest over all groups: per-row %.2e, k_ab %.2e, segment table %.2e" % (OUTPUT[which], comp, *worst))
    assert not fails, fails


@pytest.mark.parametrize("comp", COMPONENTS)
def test_consistency_with_the_density_kernels(ctx, comp):
    """liquid_density(T, p_sat, x_pure) is rho_L and vapor_density(T, p_sat, x_pure) is rho_V, to 1e-10 / dpdrho: the conditioning
    of a density root in p."""
    c, o = ctx.c, ctx.out[comp]
    sel = np.nonzero(c.keep & (c.comp == comp))[0]
    T, p = _d(c.T[sel]), _d(o["p_sat"][sel])
    x = torch.full((len(sel),), 1.0 - comp, dtype=f64, device="cuda")
    for phase, method in ((1, "liquid_density"), (0, "vapor_density")):
        eos = _model(c, c.row[sel])[0]
        rho, nans = getattr(eos, method)(T, p, x)
        assert not nans.any()
        e = np.abs(_np(rho) / ref.C_UNIT / o["rho_vl"][sel, phase] - 1.0) * o["dpdrho_vl"][sel, phase]
        print("component %d, %s at p_sat: max |rho / rho_sat - 1| dpdrho = %.2e (bar 1e-10)" % (comp, method, e.max()))
        assert e.max() <= 1e-10


def test_failures(ctx):
    """Rows that must fail inside waves of good rows: 1.5 T_top, T = NaN, +inf, 0, negative, a NaN phi.  Status 1, zero outputs,
    iters -1; the good rows carry the bits of the run without the bad ones, with the class order and without; the public
    method returns them in nans and reduces the model."""
    c = ctx.c
    n = 256
    comp_at, top_at = c.comp[ctx.perm][:n], c.T_top[ctx.perm][:n]
    for comp in COMPONENTS:
        phi, T = ctx.phi[:n].clone(), ctx.T[:n].clone()
        mine = np.nonzero(comp_at == comp)[0]
        hot = mine[[3, 20, 41, 77]]
        for j in hot:
            T[j] = 1.5 * top_at[j]
        bad = {int(mine[5]): np.nan, int(mine[30]): np.inf, int(mine[50]): 0.0, int(mine[51]): -300.0, int(mine[100]): -np.inf}
        for j, val in bad.items():
            T[j] = val
        phi[int(mine[60]), comp] = np.nan
        phi[int(mine[61]), 1 - comp] = np.inf
        rows = np.array(sorted(list(hot) + list(bad) + [int(mine[60]), int(mine[61])]))
        others = np.setdiff1d(np.arange(n), rows)
        for order in (True, None):
            r = _run(ctx, comp, n, order=order, phi=phi, T=T)
            assert _np(r["status"])[rows].all(), (comp, rows[~_np(r["status"])[rows]])
            assert (_np(r["p_sat"])[rows] == 0.0).all() and (_np(r["rho_vl"])[rows] == 0.0).all()
            assert (_np(r["dpdrho_vl"])[rows] == 0.0).all() and (_np(r["iters"])[rows] == -1).all()
            for key in KEYS:
                assert np.array_equal(_bits(r[key])[others], _bits(ctx.r[comp][key])[:n][others]), (comp, order, key)
        # the public methods: the same rows in nans, the model reduced, the values those of the kernel
        base = c.row[ctx.perm][:n]
        for which, method in enumerate(("vapor_pressure", "equilibrium_liquid_density")):
            eos = _model(c, base)[0]
            eos.phi = phi.clone()
            value, nans = getattr(eos, method)(T, component=comp)
            nn = _np(nans)
            assert nn[rows].all() and np.array_equal(nn, _np(r["status"]))
            ok = ~nn
            assert value.shape == (ok.sum(),) and eos.rows.shape[0] == ok.sum() and eos.phi.shape[0] == ok.sum()
            want = r["p_sat"] if which == 0 else r["rho_vl"][:, 1] * ref.C_UNIT
            assert np.array_equal(_bits(value), _bits(want)[ok])


@pytest.mark.parametrize("comp", COMPONENTS)
def test_shapes(ctx, comp):
    """n = 1, 127, 128, 129 and the whole set: the first n rows carry the same bits, with the class order and without; optional
    outputs that are not asked for change nothing; an empty batch returns empty outputs."""
    full = ctx.r[comp]
    for n in (1, 127, 128, 129, None):
        for order in (None, True):
            r = _run(ctx, comp, n, order=order)
            for key in KEYS:
                assert np.array_equal(_bits(r[key]), _bits(full[key])[:n]), (n, order, key)
    for want in (("p_sat",), ("rho_vl",), ("dpdrho_vl", "iters"), ()):
        r = _run(ctx, comp, 129, order=True, want=want)
        assert set(r) == set(want) | {"status"}
        for key in r:
            assert np.array_equal(_bits(r[key]), _bits(full[key])[:129]), (want, key)
    r = _run(ctx, comp, 0)
    assert all(r[key].shape[0] == 0 for key in KEYS)


def test_full_rows(oracle):
    """Molecules that fill all 8 segment and all 8 bond slots, segment indices up to 31, on the S = 32 heterogeneous table of
    tests/tools/gc_full_rows.py: four of them (none, polar, self-associating, self-associating and polar), each in either
    slot, at 0.7 x their own T_top, against the referee with the value bar."""
    from feos_torch_amd import GcPcSaftMix, native

    mols = {m[0]: m for m in fr.HETERO}
    names = ("h1", "h2", "h3", "h6")
    for nm in names:
        assert fr.type_counts(mols[nm][1], mols[nm][2]) == (8, 8)
    pairs = [(names[i], names[(i + 1) % 4]) for i in range(4)]
    tab = fr.hetero_table()
    ident = [s for s, _ in tab]
    assert len(tab) == 32 and max(ident.index(s) for nm in names for s in mols[nm][1]) == 31
    segs = [[mols[a][1], mols[b][1]] for a, b in pairs]
    bonds = [[mols[a][2], mols[b][2]] for a, b in pairs]
    kl = fr.kab_list(ident)
    phi = np.array([[1.0, 0.95], [1.05, 1.0], [0.9, 1.1], [1.0, 1.0]])
    m = ref.Rows(oracle, oracle.gc_encode(tab, segs, bonds, kl), phi)
    idx = np.tile(np.arange(4), 2)
    comp = np.repeat(np.arange(2), 4)
    T = 0.7 * ref.t_top(m, idx, comp)
    assert np.isfinite(T).all()
    want, twin = ref.solve(m, idx, comp, T), ref.solve(m, idx, comp, T, prec=0)
    assert want["ok"].all() and twin["ok"].all()
    par = tuple(torch.tensor([v[k] for _, v in tab], dtype=f64) for k in range(8))
    eos = GcPcSaftMix(ident, par, segs, bonds, kl, torch.tensor(phi, dtype=f64))
    assert int(eos.rows[:, :16].max()) == 31 and bool((eos.rows[:, 16:32] > 0).all()) and bool((eos.rows[:, 64:80] > 0).all())
    for k in COMPONENTS:
        sl = slice(4 * k, 4 * k + 4)
        r = native.gc_pure_vle(eos._table(), 32, eos.rows, eos.phi, _d(T[sl]), k)
        assert not r["status"].any()
        got = {"p_sat": _np(r["p_sat"]), "rho_v": _np(r["rho_vl"])[:, 0], "rho_l": _np(r["rho_vl"])[:, 1]}
        for name, val in got.items():
            e = np.abs(val / want[name][sl] - 1.0)
            bar = np.maximum(FLOOR, 10.0 * np.abs(twin[name][sl] / want[name][sl] - 1.0))
            print("full rows, component %d, %-5s: max relative error %.2e, largest error / bar %.3f" % (k, name, e.max(), (e / bar).max()))
            assert (e <= bar).all(), (k, name, e, bar)
        p, nans = eos.vapor_pressure(_d(T[sl]), component=k)
        assert not nans.any() and np.array_equal(_bits(p), _bits(r["p_sat"]))
