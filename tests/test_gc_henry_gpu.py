"""GPU: pcs_gc_henry and GcPcSaftMix.henrys_law_constant against the long-double referee of tests/tools/gc_henry_referee.py (the
saturation referee's solve on the solvent, the oracle's mu_s and exact VJP at (rho_L e_v); independent of the kernel).

The 3,072-row set of the saturation referee (2 solvents x 4 temperature factors x 384 rows, interleaved so that factors, solvents
and classes mix within a wave) is run once per solute; a solute's call is compared on the 1,536 rows whose temperature was made
for its solvent, the other half are its wave mates (some solve, some have a super-critical solvent).

Bars.  ln H: max(1e-10, 10 x the error of the referee's fp64 twin on the same row), absolute (the rule of tests/test_henry_gpu.py).
rho_V, rho_L, p_sat, dpdrho_l: max(1e-12, 10 x twin) relative (the rule of tests/test_gc_saturation_gpu.py).  dlnh_drho is held
through the gradient.  Gradients through the public method under seeded weights on ln H: per-row columns (phi_0, phi_1, T) 1e-10
of the row's largest exact component, k_ab records 1e-10 of the largest record, segment-table columns GRAD_TOL = 1e-7 (the bar of
the VJP kernel against the referee's Richardson table differences).  State functions at a zero partial density: mu_s against the
long-double oracle at max(1e-12, 10 x twin) of max(1, |mu_s|); their VJP with the weight on the absent component: the gradient
bars.  Consistency with derivatives / equilibrium_liquid_density: 1e-10 max(1, |rho_L dlnh_drho|), the conditioning of H in rho_L.

Measured (MI355X, solute 0 / 1): ln H 4.8e-14 / 5.9e-14, rho_V 1.7e-14 / 2.1e-14, rho_L 8.0e-15 / 6.9e-15, p_sat 1.4e-14 / 1.2e-14,
dpdrho_l 8.4e-14 / 5.9e-14 (at most 8 % of the bar); rho_V, rho_L, p_sat and the status are bit-identical to pcs_gc_pure_vle on the
solvent; 233 / 232 rows have a super-critical solute; evaluations per solved row: median 39, at most 178.  mu_s at a zero partial
density 1.9e-14 (twin 1.8e-14), its VJP per-row 2.2e-13 / 9.9e-14, k_ab 1.3e-15 / 6.8e-16, segment table 1.4e-11.  Gradients of
ln H, largest over all groups: per-row 3.3e-13 / 4.8e-14, k_ab records 7.7e-16 / 5.1e-16, segment table 1.5e-10.  Consistency
3.8e-14 / 4.6e-14; identical molecules 2.1e-14 / 2.5e-14; full rows 1.9e-14 / 1.2e-14.  The module takes 26 s, most of it the
referee's input set, which it shares with tests/test_gc_saturation_gpu.py.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import gc_henry_referee as ref  # noqa: E402
import gc_saturation_referee as sref  # noqa: E402
import gc_point_rows as gp  # noqa: E402
import gc_full_rows as fr  # noqa: E402

pytestmark = pytest.mark.gpu

SOLUTES = (0, 1)
KEYS = ("h", "rho_vl", "p_sat", "dlnh_drho", "dpdrho_l", "status", "iters")
OPTIONAL = ("rho_vl", "p_sat", "dlnh_drho", "dpdrho_l", "iters")
GRAD_TOL = 1e-7   # tests/test_gc_density_gpu.py
ROW_TOL = 1e-10
LNH_FLOOR = 1e-10
FLOOR = 1e-12
f64 = torch.float64


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

    h = ref.inputs(oracle)
    c = h.c
    g = Ctx()
    g.h, g.c = h, c
    eos = _model(c, np.arange(sref.N_ROWS))[0]
    g.table, g.S = eos._table(), eos.S
    g.perm = ref.interleave(c.n)
    g.back = np.argsort(g.perm)
    g.rows = eos.rows[_d(c.row[g.perm])].contiguous()
    g.phi, g.T = _d(c.phi[g.perm]), _d(c.T[g.perm])
    g.order = native.gc_class_order(g.table, g.S, g.rows)
    g.r = {s: native.gc_henry(g.table, g.S, g.rows, g.phi, g.T, s, order=g.order) for s in SOLUTES}
    g.out = {s: {key: _np(g.r[s][key])[g.back] for key in KEYS} for s in SOLUTES}  # in the referee's row order
    return g


def _run(g, solute, n=None, order=None, **changed):
    from feos_torch_amd import native

    sl = slice(0, n)
    args = {"phi": g.phi[sl], "T": g.T[sl]}
    args.update(changed)
    rows = g.rows[sl]
    od = native.gc_class_order(g.table, g.S, rows) if order is True else order
    return native.gc_henry(g.table, g.S, rows, args["phi"], args["T"], solute, order=od, want=changed.get("want", OPTIONAL))


def _value_errors(h, o, k):
    """{name: (error [m], bar [m])} of a launch's outputs `o` (referee order) on the rows k"""
    c = h.c
    twin = sref.twin_error(c)
    out = {"ln_h": (np.abs(np.log(o["h"][k]) - h.ln_h[k]), np.maximum(LNH_FLOOR, 10.0 * h.twin_lnh[k]))}
    got = {"rho_v": o["rho_vl"][:, 0], "rho_l": o["rho_vl"][:, 1], "p_sat": o["p_sat"], "dp_l": o["dpdrho_l"]}
    want = {"rho_v": c.rho_v, "rho_l": c.rho_l, "p_sat": c.p_sat, "dp_l": c.dp_l}
    for name in got:
        out[name] = (np.abs(got[name][k] / want[name][k] - 1.0), np.maximum(FLOOR, 10.0 * twin[name][k]))
    return out


@pytest.mark.parametrize("solute", SOLUTES)
def test_values_against_the_referee(ctx, solute):
    from feos_torch_amd import native

    h, c, o = ctx.h, ctx.c, ctx.out[solute]
    k = h.keep & (h.solute == solute)
    assert k.sum() >= 1300
    assert not o["status"][k].any(), np.nonzero(k & o["status"])[0]  # every kept row is solved
    fails = []
    for name, (e, bar) in _value_errors(h, o, k).items():
        print("solute %d, %-5s: %d rows, max error %.2e, largest error / bar %.3f" % (solute, name, k.sum(), e.max(), (e / bar).max()))
        if not (e <= bar).all():
            fails.append((name, float(e.max()), float((e / bar).max())))
    ev = o["iters"][~o["status"]]
    print("solute %d: evaluations per solved row: median %d, max %d; %d of %d rows failed (wave mates included)"
          % (solute, np.median(ev), ev.max(), o["status"].sum(), c.n))
    assert not fails, fails
    st = o["status"]
    assert (o["iters"][~st] >= 2).all() and (o["iters"][st] == -1).all()
    for key in ("h", "rho_vl", "p_sat", "dlnh_drho", "dpdrho_l"):
        assert (o[key][st] == 0.0).all(), key
    assert (o["h"][~st] > 0.0).all() and np.isfinite(o["dlnh_drho"][~st]).all()
    # reported, not a bar: the solvent's state against pcs_gc_pure_vle(component = v) on the same launch
    p = native.gc_pure_vle(ctx.table, ctx.S, ctx.rows, ctx.phi, ctx.T, 1 - solute, order=ctx.order)
    same = {"rho_vl": np.array_equal(_bits(p["rho_vl"]), _bits(ctx.r[solute]["rho_vl"])),
            "p_sat": np.array_equal(_bits(p["p_sat"]), _bits(ctx.r[solute]["p_sat"])),
            "status": np.array_equal(_np(p["status"]), _np(ctx.r[solute]["status"]))}
    print("solute %d: bit-identical to pcs_gc_pure_vle(component = %d): %s" % (solute, 1 - solute, same))


@pytest.mark.parametrize("solute", SOLUTES)
def test_supercritical_solute_is_an_ordinary_row(ctx, solute):
    h, c, o = ctx.h, ctx.c, ctx.out[solute]
    top_solute = c.t_top[solute][c.row]
    k = h.keep & (h.solute == solute) & (top_solute < c.T)
    print("solute %d: %d kept rows whose solute has no equilibrium of its own at T (T / T_top of the solute up to %.2f)"
          % (solute, k.sum(), (c.T[k] / top_solute[k]).max()))
    assert k.sum() >= 32
    assert not o["status"][k].any()
    for name, (e, bar) in _value_errors(h, o, k).items():
        assert (e <= bar).all(), (name, float((e / bar).max()))


@pytest.mark.parametrize("solute", SOLUTES)
def test_shapes(ctx, solute):
    """n = 1, 127, 128, 129 and the whole set: the first n rows carry the same bits, with the class order and without; optional
    outputs that are not asked for change nothing; an empty batch returns empty outputs."""
    full = ctx.r[solute]
    for n in (1, 127, 128, 129, None):
        for order in (None, True):
            r = _run(ctx, solute, n, order=order)
            for key in KEYS:
                assert np.array_equal(_bits(r[key]), _bits(full[key])[:n]), (n, order, key)
    for want in (("p_sat",), ("rho_vl",), ("dlnh_drho", "iters"), ("dpdrho_l",), ()):
        r = _run(ctx, solute, 129, order=True, want=want)
        assert set(r) == set(want) | {"h", "status"}
        for key in r:
            assert np.array_equal(_bits(r[key]), _bits(full[key])[:129]), (want, key)
    r = _run(ctx, solute, 0)
    assert all(r[key].shape[0] == 0 for key in KEYS)


def test_failures(ctx):
    """Rows that must fail inside waves of good rows: 1.5 T_top of the solvent, T = NaN, +-inf, 0, negative, a non-finite phi of
    either molecule.  Status 1, zero outputs, iters -1; the good rows carry the bits of the run without the bad ones, with the
    class order and without; the public method returns them in nans and reduces the model."""
    c, h = ctx.c, ctx.h
    n = 256
    solvent_at, top_at = c.comp[ctx.perm][:n], c.T_top[ctx.perm][:n]
    for solute in SOLUTES:
        phi, T = ctx.phi[:n].clone(), ctx.T[:n].clone()
        mine = np.nonzero(solvent_at == 1 - solute)[0]
        hot = mine[[3, 20, 41, 77]]
        for j in hot:
            T[j] = 1.5 * top_at[j]
        bad = {int(mine[5]): np.nan, int(mine[30]): np.inf, int(mine[50]): 0.0, int(mine[51]): -300.0, int(mine[100]): -np.inf}
        for j, val in bad.items():
            T[j] = val
        phi[int(mine[60]), solute] = np.nan
        phi[int(mine[61]), 1 - solute] = np.inf
        rows = np.array(sorted(list(hot) + list(bad) + [int(mine[60]), int(mine[61])]))
        others = np.setdiff1d(np.arange(n), rows)
        for order in (True, None):
            r = _run(ctx, solute, n, order=order, phi=phi, T=T)
            assert _np(r["status"])[rows].all(), (solute, rows[~_np(r["status"])[rows]])
            for key in ("h", "rho_vl", "p_sat", "dlnh_drho", "dpdrho_l"):
                assert (_np(r[key])[rows] == 0.0).all(), key
            assert (_np(r["iters"])[rows] == -1).all()
            for key in KEYS:
                assert np.array_equal(_bits(r[key])[others], _bits(ctx.r[solute][key])[:n][others]), (solute, order, key)
        # the public method: the same rows in nans, the model reduced, the values those of the kernel
        eos = _model(c, c.row[ctx.perm][:n])[0]
        eos.phi = phi.clone()
        value, nans = eos.henrys_law_constant(T, solute=solute)
        nn = _np(nans)
        assert nn[rows].all() and np.array_equal(nn, _np(r["status"]))
        ok = ~nn
        assert value.shape == (ok.sum(),) and eos.rows.shape[0] == ok.sum() and eos.phi.shape[0] == ok.sum()
        assert np.array_equal(_bits(value), _bits(r["h"])[ok])


@pytest.fixture(scope="module")
def zero_density(ctx):
    """mu_s from pcs_gc_derivatives at the referee's (rho_L e_v), the long-double oracle's and its fp64 evaluation's"""
    from feos_torch_amd import native

    h, c = ctx.h, ctx.c
    k = np.nonzero(h.keep)[0]
    rho = np.zeros((len(k), 2))
    rho[np.arange(len(k)), c.comp[k]] = c.rho_l[k]
    eos = _model(c, np.arange(sref.N_ROWS))[0]
    rows = eos.rows[_d(c.row[k])].contiguous()
    mu = _np(native.gc_derivatives(ctx.table, ctx.S, rows, _d(c.phi[k]), _d(c.T[k]), _d(rho))[2])
    mu64 = ref.mu_solute(c.m, c.row[k], h.solute[k], c.T[k], c.rho_l[k], prec=0)
    return k, rho, mu[np.arange(len(k)), h.solute[k]], mu64


def test_state_functions_at_a_zero_partial_density(ctx, zero_density):
    h = ctx.h
    k, _, got, mu64 = zero_density
    assert np.isfinite(got).all()
    scale = np.maximum(1.0, np.abs(h.mu_s[k]))
    e = np.abs(got - h.mu_s[k]) / scale
    twin = np.abs(mu64 - h.mu_s[k]) / scale
    bar = np.maximum(FLOOR, 10.0 * twin)
    print("mu_s of pcs_gc_derivatives at (rho_L e_v), %d rows: max error %.2e of max(1, |mu_s|) (twin %.2e), largest error / bar %.3f"
          % (len(k), e.max(), twin.max(), (e / bar).max()))
    assert (e <= bar).all()


@pytest.mark.parametrize("solute", SOLUTES)
def test_vjp_with_the_weight_on_the_absent_component(ctx, zero_density, solute):
    """pcs_gc_derivatives_vjp with g_mu on the component whose partial density is exactly zero, through GcPcSaftMix.derivatives,
    against gc_derivatives_vjp_exact: (phi_0, phi_1, T, rho_0, rho_1) per row, the k_ab records and the segment table."""
    h, c = ctx.h, ctx.c
    k_all, rho_all, _, _ = zero_density
    pick = h.solute[k_all] == solute
    k, rho = k_all[pick], rho_all[pick]
    g = np.random.default_rng(ref.SEED + 10 + solute).uniform(0.5, 1.5, len(k))
    want_row, want_seg, want_kab = ref.exact_mu(c.m, c.row[k], h.solute[k], c.T[k], c.rho_l[k], g)
    eos, cols, kab, ph = _model(c, c.row[k], grad=True)
    T = torch.tensor(c.T[k], dtype=f64, requires_grad=True)
    dens = torch.tensor(rho, dtype=f64, requires_grad=True)
    mu = eos.derivatives(T, dens)[2]
    (mu[:, solute] * _d(g).to(mu.device)).sum().backward()
    row = np.concatenate((_np(ph.grad), _np(T.grad)[:, None], _np(dens.grad)), axis=1)
    seg = np.stack([_np(col.grad) for col in cols], axis=1)
    assert np.isfinite(row).all() and np.isfinite(seg).all() and np.isfinite(_np(kab.grad)).all()
    e_row = float((np.abs(row - want_row) / np.abs(want_row).max(axis=1, keepdims=True)).max())
    rowsd = {"enc": dict(c.m.enc, counts=c.m.enc["counts"][c.row[k]]), "kab_list": c.kab_list}
    want_k = gp.kab_records(rowsd, want_kab)
    assert (want_k != 0.0).all()
    e_kab = float(np.max(np.abs(_np(kab.grad) - want_k)) / np.max(np.abs(want_k)))
    e_seg, used = gp.seg_error(rowsd, seg, want_seg)
    assert np.all(seg[~used] == 0.0)
    e_seg_max = float(np.nanmax(e_seg))
    print("VJP of mu_s at (rho_L e_v), solute %d, %d rows: per-row %.2e (bar %.0e), k_ab records %.2e (bar %.0e), segment table %.2e (bar %.0e)"
          % (solute, len(k), e_row, ROW_TOL, e_kab, ROW_TOL, e_seg_max, GRAD_TOL))
    assert e_row <= ROW_TOL and e_kab <= ROW_TOL and e_seg_max <= GRAD_TOL


@pytest.mark.parametrize("solute", SOLUTES)
def test_gradients_through_the_public_method(ctx, oracle, solute):
    """henrys_law_constant with requires_grad on the eight segment vectors, k_ab, phi and T, under the referee's seeded weights on
    ln H: for the whole set and once per model class with the weights masked to it."""
    h, c = ctx.h, ctx.c
    wt = ref.weighted(oracle, h, solute)
    sel = np.nonzero(h.solute == solute)[0]
    pos = {int(r): j for j, r in enumerate(sel)}
    eos, cols, kab, ph = _model(c, c.row[sel], grad=True)
    T = torch.tensor(c.T[sel], dtype=f64, requires_grad=True)
    value, nans = eos.henrys_law_constant(T, solute=solute)
    assert not _np(nans)[h.keep[sel]].any()
    assert not nans.any(), "the whole set solves, so the model is not reduced and value is aligned with sel"
    ln_h = torch.log(value)
    rowsd = {"enc": c.m.enc, "kab_list": c.kab_list}
    groups = {"all": np.ones(c.n, dtype=bool)}
    groups.update({gp.CLASS_NAMES[k]: c.cls == k for k in wt["groups"]})
    leaves = [*cols, kab, ph, T]
    fails, worst = [], [0.0, 0.0, 0.0]
    for gname, mask in groups.items():
        weights = np.where(mask, wt["g"], 0.0)[sel]
        for leaf in leaves:
            leaf.grad = None
        (ln_h * _d(weights).to(ln_h.device)).sum().backward(retain_graph=True)
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
        assert len(want_k) == 4 and (want_k != 0.0).any(), gname
        if gname == "all":
            assert (want_k != 0.0).all()  # every record of the set gets a gradient from the whole set
        e_kab = float(np.max(np.abs(got_k - want_k)) / np.max(np.abs(want_k)))
        sub = dict(rowsd, enc=dict(c.m.enc, counts=c.m.enc["counts"][c.row[sel]]))
        e_seg, used = gp.seg_error(sub, seg, want_seg, mask_rows=weights != 0.0)
        if not np.all(seg[~used] == 0.0):
            fails.append((gname, "segments no row uses must have zero gradient"))
        e_seg_max = float(np.nanmax(e_seg))
        print("ln H, solute %d, %-14s %5d rows: per-row %.2e (bar %.0e), k_ab records %.2e (bar %.0e), segment table %.2e (bar %.0e)"
              % (solute, gname, len(ids), e_row, ROW_TOL, e_kab, ROW_TOL, e_seg_max, GRAD_TOL))
        worst = [max(a, b) for a, b in zip(worst, (e_row, e_kab, e_seg_max))]
        if not (e_row <= ROW_TOL and e_kab <= ROW_TOL and e_seg_max <= GRAD_TOL):
            fails.append((gname, e_row, e_kab, e_seg_max))
    print("ln H, solute %d: largest over all groups: per-row %.2e, k_ab %.2e, segment table %.2e" % (solute, *worst))
    assert not fails, fails


@pytest.mark.parametrize("solute", SOLUTES)
def test_consistency_with_the_existing_methods(ctx, solute):
    """H / (rho_L k_B T) is exp(mu_s) of `derivatives` at the rho_L of `equilibrium_liquid_density`, to the conditioning of H in
    rho_L."""
    h, c, o = ctx.h, ctx.c, ctx.out[solute]
    sel = np.nonzero(h.keep & (h.solute == solute))[0]
    T = _d(c.T[sel])
    eos = _model(c, c.row[sel])[0]
    rho_l, nans = eos.equilibrium_liquid_density(T, component=1 - solute)
    assert not nans.any()
    rl = _np(rho_l) / sref.C_UNIT
    rho = np.zeros((len(sel), 2))
    rho[:, 1 - solute] = rl
    mu = _np(eos.derivatives(T, _d(rho))[2])[:, solute]
    H, nans = eos.henrys_law_constant(T, solute=solute)
    assert not nans.any() and np.array_equal(_bits(H), o["h"][sel].view(np.int64))
    e = np.abs(_np(H) * ref.P_RED / (rl * c.T[sel]) / np.exp(mu) - 1.0)
    bar = 1e-10 * np.maximum(1.0, np.abs(rl * o["dlnh_drho"][sel]))
    print("solute %d: H / (rho_L k_B T) against exp(mu_s) of derivatives at equilibrium_liquid_density: max %.2e, largest error / bar %.3f"
          % (solute, e.max(), (e / bar).max()))
    assert (e <= bar).all()


@pytest.mark.parametrize("solute", SOLUTES)
def test_identical_molecules_give_the_pure_fugacity(ctx, oracle, solute):
    """A row of two identical molecules without binary segment records is the pure fluid in both slots: the solute's fugacity at
    infinite dilution in the saturated liquid is the liquid's own, which equals the saturated vapour's, so
    ln H = ln f_V = ln(rho_V k_B T) + mu(rho_V) with mu from `derivatives` on the vapour -- a phase the Henry kernel does not
    evaluate.  Bar: the value bar, max(1e-10, 10 x twin) with the referee's twin on these rows; the referee's own ln H is
    compared too."""
    from feos_torch_amd import GcPcSaftMix, native

    c = ctx.c
    v = 1 - solute
    pick = np.arange(0, sref.N_ROWS, 3)
    tab = gp.table()
    cols = tuple(torch.tensor([w[k] for _, w in tab], dtype=f64) for k in range(8))
    segs = [[c.segment_lists[i][v]] * 2 for i in pick]
    bonds = [[c.bond_lists[i][v]] * 2 for i in pick]
    phi = np.stack((c.m.phi[pick, v],) * 2, axis=1)
    Tn = 0.7 * c.t_top[v][pick]
    m = sref.Rows(oracle, oracle.gc_encode(tab, segs, bonds, []), phi)
    idx, sol = np.arange(len(pick)), np.full(len(pick), solute)
    want, twin = ref.solve(m, idx, sol, Tn), ref.solve(m, idx, sol, Tn, prec=0)
    assert want["ok"].all() and twin["ok"].all()
    bar = np.maximum(LNH_FLOOR, 10.0 * np.abs(twin["ln_h"] - want["ln_h"]))
    eos = GcPcSaftMix([s for s, _ in tab], cols, segs, bonds, [], torch.tensor(phi, dtype=f64))
    T = _d(Tn)
    r = native.gc_henry(eos._table(), eos.S, eos.rows, eos.phi, T, solute)
    assert not r["status"].any()
    rv = _np(r["rho_vl"])[:, 0]
    rho = np.zeros((len(pick), 2))
    rho[:, v] = rv
    mu_v = _np(eos.derivatives(T, _d(rho))[2])[:, v]
    ln_fv = np.log(rv * Tn / ref.P_RED) + mu_v
    ln_h = np.log(_np(r["h"]))
    e, e_ref = np.abs(ln_h - ln_fv), np.abs(ln_h - want["ln_h"])
    print("identical molecules, solute %d, %d rows: max |ln H - ln f_V| = %.2e, max |ln H - ln H_ref| = %.2e, largest error / bar %.3f"
          % (solute, len(pick), e.max(), e_ref.max(), max((e / bar).max(), (e_ref / bar).max())))
    assert (e <= bar).all() and (e_ref <= bar).all()


def test_full_rows(oracle):
    """Molecules that fill all 8 segment and all 8 bond slots, segment indices up to 31, on the S = 32 heterogeneous table of
    tests/tools/gc_full_rows.py: four of them (none, polar, self-associating, self-associating and polar), each as solvent and as
    solute, at 0.7 x the solvent's T_top, against the referee with the value bar."""
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
    m = sref.Rows(oracle, oracle.gc_encode(tab, segs, bonds, kl), phi)
    idx = np.tile(np.arange(4), 2)
    solute = np.repeat(np.arange(2), 4)
    T = 0.7 * sref.t_top(m, idx, 1 - solute)
    assert np.isfinite(T).all()
    want, twin = ref.solve(m, idx, solute, T), ref.solve(m, idx, solute, T, prec=0)
    assert want["ok"].all() and twin["ok"].all()
    par = tuple(torch.tensor([v[k] for _, v in tab], dtype=f64) for k in range(8))
    eos = GcPcSaftMix(ident, par, segs, bonds, kl, torch.tensor(phi, dtype=f64))
    assert int(eos.rows[:, :16].max()) == 31 and bool((eos.rows[:, 16:32] > 0).all()) and bool((eos.rows[:, 64:80] > 0).all())
    for s in SOLUTES:
        sl = slice(4 * s, 4 * s + 4)
        r = native.gc_henry(eos._table(), 32, eos.rows, eos.phi, _d(T[sl]), s)
        assert not r["status"].any()
        e = np.abs(np.log(_np(r["h"])) - want["ln_h"][sl])
        bar = np.maximum(LNH_FLOOR, 10.0 * np.abs(twin["ln_h"][sl] - want["ln_h"][sl]))
        print("full rows, solute %d: max |ln H - ln H_ref| = %.2e, largest error / bar %.3f" % (s, e.max(), (e / bar).max()))
        assert (e <= bar).all(), (s, e, bar)
        for name, val in (("rho_v", _np(r["rho_vl"])[:, 0]), ("rho_l", _np(r["rho_vl"])[:, 1]), ("p_sat", _np(r["p_sat"]))):
            e = np.abs(val / want[name][sl] - 1.0)
            bar = np.maximum(FLOOR, 10.0 * np.abs(twin[name][sl] / want[name][sl] - 1.0))
            assert (e <= bar).all(), (s, name, e, bar)
        H, nans = eos.henrys_law_constant(_d(T[sl]), solute=s)
        assert not nans.any() and np.array_equal(_bits(H), _bits(r["h"]))
