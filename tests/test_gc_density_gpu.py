"""GPU: pcs_gc_density and GcPcSaftMix.liquid_density / vapor_density against the long-double referee of
tests/tools/gc_density_referee.py (root definitions restated there on a fixed packing-fraction grid, independent of the
kernel).  Each test mirrors the one of the same name in tests/test_mix_density_gpu.py.

Bars (none is new).  Values: |rho / rho_ref - 1| <= 1e-10 on every kept row, the project's bar for values against the
long-double oracle; dpdrho 1e-9.  Gradients: GRAD_TOL = 1e-7 of tests/test_gc_state_gpu.py, the project's bar for this very VJP
kernel against this very referee (whose table entries are Richardson differences, and which has no fp64 twin): per-row columns
(phi_0, phi_1, T, p, x) relative to the row's largest exact component, the k_ab records relative to the largest record, each
segment-table column relative to the column's largest reported entry (gc_point_rows.seg_error), for the whole set and once
per model class with the weights masked to it.  Input set: 5,760 liquid + 3,456 vapour rows.

One departure from the mixture test, in test_autograd: "one input alone gives the same bits" holds for k_ab, phi, T, p and
x; the eight segment vectors are column sums that pcs_gc_derivatives_vjp reduces with floating-point atomic additions whose
order is not fixed, so two calls agree to rounding, not bit for bit (tests/test_gc_state_gpu.py holds the same sums to 1e-12
of the column's largest entry across schedules; the same measure is used here).

Measured (MI355X): liquid max |rho/rho_ref - 1| 1.3e-15, dpdrho 8.0e-14; vapour 5.6e-16 / 4.4e-16; 4 - 8 / 1 - 4 evaluations per
row.  Gradients, largest over all groups: per-row columns 7.9e-14 (liquid) / 1.2e-13 (vapour) of the row maximum, k_ab records
6.1e-15 / 1.1e-15, segment-table columns 1.3e-11 / 6.1e-11.  Autograd against the kernel-level gradient 2.3e-16 per row, 1.9e-15 on
the segment table.  Round trip 2.8e-14 (bubble) / 1.4e-14 (dew).  The module takes 15 s.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import gc_density_referee as ref  # noqa: E402
import gc_point_rows as gp  # noqa: E402

pytestmark = pytest.mark.gpu

PHASES = (ref.LIQUID, ref.VAPOUR)
WORKGROUP = 128  # GDBLOCK of csrc/gc_density.hip
SHAPES = (1, 63, 64, 65, WORKGROUP - 1, WORKGROUP, WORKGROUP + 1, 5 * WORKGROUP + 17)
KEYS = ("rho", "dpdrho", "status", "iters")
ROW_COLUMNS = ("phi_0", "phi_1", "T", "p", "x")
GRAD_TOL = 1e-7  # tests/test_gc_state_gpu.py
C_UNIT = 1.0 / (1e3 * (6.02214076e23 * (1e-10 * 1e-10 * 1e-10)))  # A^-3 -> kmol/m3
f64 = torch.float64
name = lambda phase: "vapour" if phase else "liquid"


class Ctx:
    pass


def _d(x):
    return torch.from_numpy(np.array(x)).cuda()  # (a copy: the input set's arrays are read-only)


def _np(x):
    return x.detach().cpu().numpy()


def _bits(x):
    x = _np(x)
    return x.view(np.int64) if x.dtype == np.float64 else x


def _model(base, rows, grad=False):
    """GcPcSaftMix on the rows `rows` of the base set -> (model, segment vectors, k_ab record tensor, phi)"""
    from feos_torch_amd import GcPcSaftMix

    tab = gp.table()
    cols = [torch.tensor([v[k] for _, v in tab], dtype=f64, requires_grad=grad) for k in range(8)]
    kab = torch.tensor([k[2] for k in base.kab_list], dtype=f64, requires_grad=grad)
    kl = [(k[0], k[1], kv) for k, kv in zip(base.kab_list, kab)]
    ph = torch.tensor(base.phi[rows], dtype=f64, requires_grad=grad)
    eos = GcPcSaftMix([s for s, _ in tab], tuple(cols), [base.segment_lists[i] for i in rows], [base.bond_lists[i] for i in rows], kl, ph)
    return eos, cols, kab, ph


def kernel_gradient(table, S, rows, ph, T, p, x, rho, dpdrho, g):
    """The gradient of sum_i g_i rho_i [A^-3] the way _GcDensity forms it: one native.gc_derivatives_vjp call with
    g_p = w = -g / dpdrho and no other weight -> row [n,5] (phi_0, phi_1, T, p, x), kab [S,S], seg [S,8] (GPU tensors).  kab is
    the gradient w.r.t. the symmetric pair, stored at both places as the referee does: a binary segment record fills
    k_ab[a,b] and k_ab[b,a] (gc_pcsaft._kab_matrix), so autograd hands it the sum of both entries of _kab_gradient."""
    from feos_torch_amd import native
    from feos_torch_amd.gc_pcsaft import _kab_gradient, _phi_gradient

    w = -g / dpdrho
    gseg, jac9, agg = native.gc_derivatives_vjp(table, S, rows, ph, T, torch.stack((x * rho, (1.0 - x) * rho), dim=1), g_p=w)
    unit = ref.P_RED / T
    row = torch.cat((_phi_gradient(jac9, agg, ph), (jac9[:, 6] + w * p * unit / T)[:, None], (-w * unit)[:, None],
                     (rho * (jac9[:, 7] - jac9[:, 8]))[:, None]), dim=1)
    gk = _kab_gradient(table, S, rows, ph, T, jac9[:, 1], jac9[:, 4])
    return row, gk + gk.t(), gseg


@pytest.fixture(scope="module")
def ctx(oracle, hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from feos_torch_amd import native

    out = {}
    for phase in PHASES:
        c = ref.inputs(oracle, phase)
        g = Ctx()
        g.c, g.phase = c, phase
        eos = _model(c.base, np.arange(c.base.n))[0]
        g.table, g.S = eos._table(), eos.S
        g.perm = ref.interleave(c.n, c.nblocks)  # classes, temperature and pressure blocks mix within a wave
        g.back = np.argsort(g.perm)
        g.rows = eos.rows[_d(c.row[g.perm])].contiguous()
        g.dev = [_d(v[g.perm]) for v in (c.phi, c.T, c.p, c.x)]
        g.order = native.gc_class_order(g.table, g.S, g.rows)
        g.r = native.gc_density(g.table, g.S, g.rows, *g.dev, phase, order=g.order)
        g.rho, g.dpdrho, g.status, g.iters = (_np(g.r[k])[g.back] for k in KEYS)
        out[phase] = g
    return out


def _run(g, n=None, order=None, table=None, S=None, **changed):
    from feos_torch_amd import native

    sl = slice(0, n)
    args = dict(zip(("phi", "T", "p", "x"), (v[sl] for v in g.dev)))
    args.update(changed)
    table, S = (g.table, g.S) if table is None else (table, S)
    rows = g.rows[sl]
    od = native.gc_class_order(table, S, rows) if order is True else order
    return native.gc_density(table, S, rows, args["phi"], args["T"], args["p"], args["x"], g.phase, order=od)


@pytest.mark.parametrize("phase", PHASES)
def test_values_against_the_referee(ctx, phase):
    g = ctx[phase]
    c, k = g.c, g.c.keep
    assert not g.status[k].any(), np.nonzero(k & g.status)[0]
    e_rho = np.abs(g.rho[k] / c.rho[k] - 1.0)
    e_dp = np.abs(g.dpdrho[k] / c.dpdrho[k] - 1.0)
    ev = g.iters[~g.status]
    print("%s: %d kept rows of %d, max |rho/rho_ref - 1| = %.2e (bar 1e-10), max |dpdrho/ref - 1| = %.2e (bar 1e-9); evaluations "
          "per converged row: median %d, max %d, histogram %s; %d rows failed" % (
              name(phase), k.sum(), c.n, e_rho.max(), e_dp.max(), np.median(ev), ev.max(), np.bincount(ev).tolist(), g.status.sum()))
    assert e_rho.max() <= 1e-10
    assert e_dp.max() <= 1e-9
    assert (g.iters[~g.status] >= 1).all() and (g.iters[g.status] == -1).all()
    assert (g.rho[g.status] == 0.0).all() and (g.dpdrho[g.status] == 0.0).all()
    # where the referee decides that there is no root on the branch, the kernel returns none either
    gone = (c.status == ref.ENDS) | (c.status == ref.NONE)
    assert g.status[gone].all()


def test_failure_mask(ctx):
    """One invalid row per rule inside waves of valid rows: status 1, zero outputs, iters -1, neighbours bit-identical to the run
    without them; the pure-limit blocks (x = 0, x = 1) converge."""
    g = ctx[ref.LIQUID]
    n = 256
    phi, T, p, x = (v[:n].clone() for v in g.dev)
    bad = {5: (0, np.nan), 37: (0, np.inf), 70: (0, 0.0), 71: (0, -300.0), 100: (1, np.nan), 129: (1, np.inf), 130: (1, 0.0),
           163: (1, -1e5), 190: (2, np.nan), 200: (2, -1e-3), 201: (2, 1.0 + 1e-9), 255: (2, np.inf)}
    for row, (which, value) in bad.items():
        (T, p, x)[which][row] = value
    phi[222, 1] = np.nan
    r = _run(g, n, order=True, phi=phi, T=T, p=p, x=x)
    rows = np.array(sorted(list(bad) + [222]))
    others = np.setdiff1d(np.arange(n), rows)
    assert _np(r["status"])[rows].all()
    assert (_np(r["rho"])[rows] == 0.0).all() and (_np(r["dpdrho"])[rows] == 0.0).all() and (_np(r["iters"])[rows] == -1).all()
    for key in KEYS:
        assert np.array_equal(_bits(r[key])[others], _bits(g.r[key])[:n][others]), key
    # x = 0 and x = 1 are valid: the pure-limit blocks of the liquid set converge
    c = g.c
    ends = c.keep & ((c.x == 0.0) | (c.x == 1.0))
    assert ends.sum() >= 2000 and not g.status[ends].any()


def test_pressure_above_the_vapour_branch_fails(ctx, oracle):
    """Vapour at 50 x the dew pressure, rows at 1.2 T_batch: where the referee reports that the branch ends below p_spec the
    kernel fails too -- it never returns the liquid root -- each such row inside a wave of valid rows."""
    from feos_torch_amd import native

    g = ctx[ref.VAPOUR]
    c = g.c
    rows = np.nonzero(c.keep & (c.block == 0) & (c.factor == 2))[0]
    p50 = 50.0 * c.p[rows]
    want, slope, st = ref.solve(c.m, c.row[rows], c.T[rows], p50, c.x[rows], ref.VAPOUR, exact_slope=False)[:3]
    gone = st == ref.ENDS
    print("vapour at 50 x p_dew, 1.2 T_batch: the referee reports 'branch ends' for %d of %d rows" % (gone.sum(), len(rows)))
    assert gone.sum() >= 10
    # a wave-mixed batch: the valid rows at their own pressure, every third one at 50 x
    pick = np.arange(len(rows)) % 3 == 0
    p = np.where(pick, p50, c.p[rows])
    pos = _d(g.back[rows])
    dev_rows = g.rows[pos].contiguous()
    r = native.gc_density(g.table, g.S, dev_rows, _d(c.phi[rows]), _d(c.T[rows]), _d(p), _d(c.x[rows]), ref.VAPOUR)
    status, rho = _np(r["status"]), _np(r["rho"])
    assert status[pick & gone].all() and (rho[pick & gone] == 0.0).all()
    assert not status[~pick].any()
    assert np.array_equal(rho[~pick].view(np.int64), g.rho[rows][~pick].view(np.int64))
    # and the rows with a root at 50 x agree with the referee's
    with np.errstate(invalid="ignore"):
        tight = pick & (st == ref.OK) & (slope >= ref.MIN_SLOPE)
    assert not status[tight].any()
    assert np.abs(rho[tight] / want[tight] - 1.0).max(initial=0.0) <= 1e-10


@pytest.mark.parametrize("phase", PHASES)
def test_shapes(ctx, phase):
    """Prefixes of the big batch -- below, at and past one wave / workgroup, several workgroups with a ragged tail -- carry the
    bits of the same rows inside it, with the class order and without; an empty batch returns empty outputs; the table padded
    with unused segment types to S = 32 gives the same bits."""
    from feos_torch_amd.gc_pcsaft import build_table

    g = ctx[phase]
    for n in sorted(set(SHAPES)):
        for order in (None, True):
            r = _run(g, n, order=order)
            for key in KEYS:
                assert r[key].shape == (n,)
                assert np.array_equal(_bits(r[key]), _bits(g.r[key])[:n]), (n, order, key)
    r = _run(g, 0)
    assert all(r[key].shape == (0,) for key in KEYS)
    plain = _run(g, order=None)
    for key in KEYS:
        assert np.array_equal(_bits(plain[key]), _bits(g.r[key])), key
    # the table padded with unused segment types to S = 32 (the largest table: the LDS of one workgroup must still fit)
    S = g.S
    assert S < 32
    seg = g.table[: S * 8].view(S, 8)
    kab = 1.0 - g.table[S * 8 + 2 * S * S:].view(S, S)
    seg32 = torch.cat((seg, seg[:1].repeat(32 - S, 1)))
    kab32 = torch.zeros((32, 32), dtype=f64, device=seg.device)
    kab32[:S, :S] = kab
    for order in (True, None):
        padded = _run(g, order=order, table=build_table(seg32, kab32), S=32)
        for key in KEYS:
            assert np.array_equal(_bits(padded[key]), _bits(g.r[key])), (order, key)


@pytest.mark.parametrize("phase", PHASES)
def test_gradients(ctx, oracle, phase):
    """The kernel-level gradient, formed the way _GcDensity forms it, against the referee on the kept rows: for the whole set and
    once per model class with the weights masked to it (gc_point_rows.groups).  Bar: GRAD_TOL for every group."""
    g = ctx[phase]
    c = g.c
    wt = ref.weighted(oracle, c)
    rowsd = {"enc": c.m.enc, "kab_list": c.base.kab_list}
    failed = _d(g.status)
    dev = [_d(v) for v in (c.phi, c.T, c.p, c.x)]
    rows_dev = g.rows[_d(g.back)].contiguous()  # block-major, as the referee's arrays
    rho = torch.where(failed, torch.full((c.n,), 5e-3, dtype=f64, device="cuda"), _d(g.rho))
    dp = torch.where(failed, torch.ones((c.n,), dtype=f64, device="cuda"), _d(g.dpdrho))
    groups = {"all": np.ones(c.n, dtype=bool)}
    groups.update({gp.CLASS_NAMES[k]: c.cls == k for k in wt["groups"]})
    fails, n_zero = [], 0
    for gname, mask in groups.items():
        weights = np.where(mask & ~g.status, wt["g"], 0.0)
        row, kab, seg = (_np(t) for t in kernel_gradient(g.table, g.S, rows_dev, *dev, rho, dp, _d(weights)))
        assert np.isfinite(row).all() and np.isfinite(kab).all() and np.isfinite(seg).all(), gname
        if gname == "all":
            want_kab, want_seg = wt["all"]["grad_kab"], wt["all"]["grad_seg"]
            sel = np.concatenate([v["rows"] for v in wt["groups"].values()])
            want_phi = np.concatenate([v["phi"] for v in wt["groups"].values()])
        else:
            v = wt["groups"][[k for k in wt["groups"] if gp.CLASS_NAMES[k] == gname][0]]
            want_kab, want_seg, sel, want_phi = v["grad_kab"], v["grad_seg"], v["rows"], v["phi"]
        # per-row columns, relative to the row's largest exact component
        want_row = wt["g"][sel, None] * c.grad_row[sel]
        want_row[:, :2] = want_phi  # the phi columns of the second call
        e_row = np.abs(row[sel] - want_row) / np.abs(want_row).max(axis=1, keepdims=True)
        off = np.ones(c.n, dtype=bool)
        off[sel] = False
        assert (row[off & ~g.status] == 0.0).all(), gname  # rows without weight carry no gradient
        # the k_ab records, relative to the largest record
        got_k, want_k = gp.kab_records(rowsd, kab), gp.kab_records(rowsd, want_kab)
        e_kab = float(np.max(np.abs(got_k - want_k)) / np.max(np.abs(want_k)))
        for j in np.nonzero(want_k == 0.0)[0]:
            n_zero += 1
            if got_k[j] != 0.0:
                fails.append((gname, "k_ab record %d must be exactly zero" % j, float(got_k[j])))
        # the segment table, per column relative to the column's largest reported entry
        sub = dict(rowsd, enc=dict(c.m.enc, counts=c.m.enc["counts"][c.row]))
        e_seg, used = gp.seg_error(sub, seg, want_seg, mask_rows=weights != 0.0)
        if not np.all(seg[~used] == 0.0):
            fails.append((gname, "segments no row uses must have zero gradient"))
        for j in range(8):
            if np.isnan(e_seg[j]) and (want_seg[:, j] == 0.0).all():  # a column the referee leaves identically zero
                n_zero += 1
                if not (seg[:, j] == 0.0).all():
                    fails.append((gname, "segment column %d must be exactly zero" % j, float(np.abs(seg[:, j]).max())))
        print("%s gradients, %-14s %5d rows: per-row %s; k_ab records %.2e; segment table %s" % (
            name(phase), gname, len(sel), " ".join("%s %.1e" % (n_, e) for n_, e in zip(ROW_COLUMNS, e_row.max(axis=0))), e_kab,
            " ".join("-" if np.isnan(e) else "%.1e" % e for e in e_seg)))
        worst = max(float(e_row.max()), e_kab, float(np.nanmax(e_seg)))
        if not worst <= GRAD_TOL:
            fails.append((gname, "error above GRAD_TOL", worst))
    print("%s gradients: %d (group, column / record) pairs exactly zero" % (name(phase), n_zero))
    assert not fails, fails


def _seg_close(a, b):
    """two segment-vector gradients [S] x 8 agree to 1e-12 of each column's largest entry (atomic reduction: see the module docstring)"""
    return all(float((x - y).abs().max()) <= 1e-12 * float(y.abs().max()) for x, y in zip(a, b))


@pytest.mark.parametrize("phase", PHASES)
def test_autograd(ctx, phase):
    """liquid_density / vapor_density with requires_grad on every input, on a batch in which rows fail: the gradients of the
    kept rows are the kernel-level ones, those of dropped rows are zero, the model is reduced; one input alone works."""
    g = ctx[phase]
    c = g.c
    n = 320
    base_rows = c.row[g.perm][:n]
    phi, T, p, x = (v[:n].clone() for v in g.dev)
    T[7], p[64], x[130] = np.nan, -1.0, 2.0
    planted = [7, 64, 130]
    if phase == ref.VAPOUR:
        p[200] = p[200] * 1e4  # far above the vapour branch
        planted.append(200)

    def fresh(needs):
        """model and leaves (8 segment vectors, k_ab records, phi, T, p, x); needs: which of the 5 groups require a gradient"""
        eos, cols, kab, _ = _model(c.base, base_rows, grad=False)
        for col in cols:
            col.requires_grad_(needs[0])
        kab.requires_grad_(needs[1])
        eos = _model_from(c.base, base_rows, cols, kab, phi.clone().requires_grad_(needs[2]))
        rest = [v.clone().requires_grad_(needs[3 + k]) for k, v in enumerate((T, p, x))]
        return eos, cols, kab, eos.phi, rest

    call = lambda m, *a: (m.vapor_density if phase else m.liquid_density)(*a)
    eos, cols, kab, ph, rest = fresh([True] * 6)
    rho, nans = call(eos, *rest)
    nans_np = _np(nans)
    expected = _np(g.r["status"])[:n].copy()
    expected[planted] = True
    assert nans_np[planted].all() and np.array_equal(nans_np, expected)
    ok = ~nans_np
    assert rho.shape == (ok.sum(),) and eos.rows.shape[0] == ok.sum() and eos.phi.shape[0] == ok.sum() and eos._order is None
    assert not nans.requires_grad
    assert np.array_equal(_bits(rho), _bits(g.r["rho"][:n] * C_UNIT)[ok])
    w = torch.linspace(0.5, 1.5, int(ok.sum()), dtype=f64, device=rho.device)
    (rho * w).sum().backward()
    got_row = np.concatenate([_np(ph.grad)] + [_np(v.grad)[:, None] for v in rest], axis=1)
    assert (got_row[~ok] == 0.0).all(), "dropped rows receive exactly zero gradient"
    # the kernel-level gradient of the same weights
    okd = _d(ok)
    weights = torch.zeros(n, dtype=f64, device="cuda")
    weights[okd] = w.cuda() * C_UNIT
    safe_rho = torch.where(okd, g.r["rho"][:n], torch.full((n,), 5e-3, dtype=f64, device="cuda"))
    safe_dp = torch.where(okd, g.r["dpdrho"][:n], torch.ones((n,), dtype=f64, device="cuda"))
    safe = [torch.where(okd, a, b) for a, b in zip((T, p, x), (v[:n] for v in g.dev[1:]))]
    row, kabm, seg = kernel_gradient(g.table, g.S, g.rows[:n], g.dev[0][:n], *safe, safe_rho, safe_dp, weights)
    row, kabm, seg = _np(row), _np(kabm), _np(seg)
    e_row = (np.abs(got_row[ok] - row[ok]).max(axis=1) / np.abs(row[ok]).max(axis=1)).max()
    rowsd = {"enc": c.m.enc, "kab_list": c.base.kab_list}
    want_k = gp.kab_records(rowsd, kabm)
    e_kab = np.abs(_np(kab.grad) - want_k).max() / np.abs(want_k).max()
    got_seg = np.stack([_np(col.grad) for col in cols], axis=1)
    e_seg = (np.abs(got_seg - seg).max(axis=0) / np.abs(seg).max(axis=0)).max()
    print("%s autograd: %d of %d rows kept, largest difference to the kernel-level gradient: per row %.2e of the row maximum, k_ab "
          "%.2e, segment table %.2e of the column maximum" % (name(phase), ok.sum(), n, e_row, e_kab, e_seg))
    assert max(e_row, e_kab, e_seg) <= 1e-12  # the same kernel results, combined in another order: a few roundings
    # one input group alone
    for j in range(6):
        eos1, cols1, kab1, ph1, rest1 = fresh([k == j for k in range(6)])
        r1, _ = call(eos1, *rest1)
        (r1 * w).sum().backward()
        leaves1, leaves = (cols1, kab1, ph1, *rest1), (cols, kab, ph, *rest)
        for k, (a, b) in enumerate(zip(leaves1, leaves)):
            if k != j:
                assert all(v.grad is None for v in (a if k == 0 else [a])), (j, k)
            elif k == 0:
                assert _seg_close([v.grad for v in a], [v.grad for v in b])
            else:
                assert np.array_equal(_bits(a.grad), _bits(b.grad)), j
    # no graph when nothing requires a gradient
    eos0 = fresh([False] * 6)[0]
    r0, _ = call(eos0, T, p, x)
    assert not r0.requires_grad and np.array_equal(_bits(r0), _bits(rho))


def _model_from(base, rows, cols, kab, ph):
    from feos_torch_amd import GcPcSaftMix

    tab = gp.table()
    kl = [(k[0], k[1], kv) for k, kv in zip(base.kab_list, kab)]
    return GcPcSaftMix([s for s, _ in tab], tuple(cols), [base.segment_lists[i] for i in rows], [base.bond_lists[i] for i in rows], kl, ph)


def test_round_trip_with_bubble_and_dew_point():
    """liquid_density(T, p_bubble, x) at the pressure bubble_point returns on gc_batch(192): the density is that call's own liquid
    to 1e-10, and the pressure of `derivatives` at it is p_bubble within 1e-10 max(p_bubble, rho) in reduced units (the measure of
    tests/test_mix_density_gpu.py: relative to p_bubble itself no fp64 evaluation of a liquid can be held; that figure is
    printed).  vapor_density(T, p_dew, y) equals the dew call's own vapour to 1e-10."""
    from feos_torch_amd import GcPcSaftMix, native
    from feos_torch_amd.synthetic import gc_batch

    tab = gp.table()
    b = gc_batch(192, tab, seed=2045)
    par = tuple(torch.tensor([v[k] for _, v in tab], dtype=f64) for k in range(8))
    make = lambda: GcPcSaftMix([s for s, _ in tab], par, b["segment_lists"], b["bond_lists"], b["kab_list"], _d(b["phi"]))
    T, x, p0 = _d(b["T"]), _d(b["x"]), _d(b["p_init"])
    for dew in (False, True):
        eos = make()
        p_b, nans = (eos.dew_point if dew else eos.bubble_point)(T, x, p0)
        T_ok, x_ok = T[~nans], x[~nans]
        point = native.gc_bubble_dew(eos._table(), eos.S, eos.rows, eos.phi, T_ok, x_ok, p0[~nans], dew)
        rho, nans2 = (eos.vapor_density if dew else eos.liquid_density)(T_ok, p_b, x_ok)
        assert not nans2.any() and rho.shape == p_b.shape and len(T_ok) >= 170
        rho_a = rho / C_UNIT
        own = point["rho4"][:, 0:2] if dew else point["rho4"][:, 2:4]
        e_rho = _np((rho_a / own.sum(dim=1) - 1.0).abs()).max()
        p_red = eos.derivatives(T_ok, torch.stack((x_ok * rho_a, (1.0 - x_ok) * rho_a), dim=1))[1]
        want = p_b * ref.P_RED / T_ok
        e_p = _np(((p_red - want).abs() / torch.maximum(want, rho_a))).max()
        e_rel = _np((p_red / want - 1.0).abs()).max()
        print("round trip, %s: %d rows, max |rho / rho_own - 1| = %.2e (bar 1e-10), max |p(rho x) - p| / max(p, rho) = %.2e "
              "(bar 1e-10), relative to p %.2e" % ("dew" if dew else "bubble", len(T_ok), e_rho, e_p, e_rel))
        assert e_rho <= 1e-10
        assert e_p <= 1e-10
