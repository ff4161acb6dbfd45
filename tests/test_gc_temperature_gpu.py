"""GPU: GcPcSaftMix.bubble_temperature / dew_temperature and pcs_gc_bubble_dew_temperature on the input set of
tests/tools/gc_temperature_referee.py: 384 gc rows (classes 0, 1, 2, 3, 5, 6) x 3 temperature factors = 1152 rows per problem,
p_spec = the long-double oracle's pressure at T_grid (the exact answer is T_grid), three starts on every row (T_grid,
0.93 T_grid, 1.07 T_grid), two row orders (as built, interleaved), with the class order of native.gc_class_order and without.

Bars, as tests/test_mix_temperature_gpu.py.  e = the largest relative deviation of the EXISTING native.gc_bubble_dew pressure
at T_grid from the oracle's, per (class, factor, problem) cell; bar_T = max(1e-10, 10 e) (T inherits at most the relative error
of p, d ln p / d ln T > 1); bar_rho = max(1e-10, bar_T x the cell's largest d ln rho / d ln p along the line).  Must-solve set:
the rows the oracle keeps AND the existing native.gc_bubble_dew solves at T_grid, 0.93 and 1.07 T_grid; it must be >= 90 % of
every cell, asserted before the new kernel runs.  Gradients: phi and p per row relative to the row's largest component,
max(1e-10, 10 x the oracle's fp64 quotient against its exact one); the k_ab records by the same rule on the record sum; the
segment table per column, max(1e-10, 10 seg_self_error) of the column's largest entry (gc_point_rows.seg_error).

  1. values  2. masks  3. bad p_spec / t_init / z / phi flagged, wave mates bit-identical  4. never wrong (the oracle's
  pressure at the returned T is p_spec within max(15, d ln p / d ln T) x bar_T)  5. schedule independence, bit for bit (orders,
  prefixes, with / without `order`, table padded to S = 32)  6. start independence (2 x bar_T)  7. gradients through the API
  8. round trip through bubble_point / dew_point (15 x bar_T)  9. shell conventions

phi = 0 is a legal (if unphysical) input of the model and phi < 0 gives a NaN model that no trial solves; the kernel flags
non-finite phi at once, and the test plants NaN, +-inf and -1 there (all must come back failed).

Measured on the MI355X (both row orders identical).  The existing pressure kernel solves all 1152 rows of both problems at all
three temperatures, so must-solve = kept = 1152.  e, largest cell: bubble 2.1e-14, dew 1.6e-13, so every bar_T is at the 1e-10
floor; bar_rho <= 5.0e-10 (bubble) / 1.3e-10 (dew).  All rows solved from all three starts.  |T / T_grid - 1|: 1.5e-16 from
T_grid (1 trial), bubble 1.2e-13 / 1.4e-13 and dew 4.1e-14 / 7.6e-14 from 0.93 / 1.07 T_grid (median 6 trials with the
confirming one; max 6 bubble, 7 dew).  rho4: bubble 3.7e-12, dew 7.6e-13.  Oracle p(T) against p_spec: <= 1.0e-12.  The three
starts agree on T within 1.4e-13.  Gradients from 0.93 T_grid: phi and p per row, relative to the row's largest component,
bubble 1.6e-13 (the oracle's fp64 quotient against its exact one 2.1e-14), dew 5.0e-13 (1.8e-15); dT/dp on its own 7.9e-13 /
6.1e-13; k_ab records 2.1e-15 / 1.8e-16; segment table, error (bar) per column m, sigma, epsilon_k, mu, kappa_ab,
epsilon_k_ab, na, nb:
  bubble 4.6e-11 (6.0e-10) 2.4e-10 (2.6e-09) 8.4e-12 (1.0e-10) 1.1e-11 (1.0e-10) 6.5e-12 (1.0e-10) 4.9e-12 (1.0e-10) 1.2e-13 (1.0e-10) 3.1e-14 (1.0e-10)
  dew    1.2e-10 (1.3e-09) 1.5e-10 (1.5e-09) 8.1e-12 (1.0e-10) 3.6e-12 (1.0e-10) 2.5e-12 (1.0e-10) 1.9e-13 (1.0e-10) 3.2e-14 (1.0e-10) 4.9e-14 (1.0e-10)
Round trip through bubble_point / dew_point: 1.0e-12 / 8.0e-13.  The whole module takes 6 s.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import gc_point_rows as gp  # noqa: E402
import gc_temperature_referee as ref  # noqa: E402

pytestmark = pytest.mark.gpu

PROBLEMS = (False, True)
ORDERS = ("as built", "interleaved")
PREFIXES = (1, 63, 64, 65, 127, 128, 129, 257)
KEYS = ("t", "rho4", "status", "iters")
f64 = torch.float64
name = lambda dew: "dew" if dew else "bubble"


class Ctx:
    pass


def _d(x):
    return torch.from_numpy(np.array(x)).cuda()  # (a copy: the input set's arrays are read-only)


def _rel(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(a - b) / np.abs(b)


def _model(c, idx, grad=False, device="cpu"):
    """GcPcSaftMix on the rows idx of the input set -> (model, segment vectors, k_ab record tensor, phi)"""
    from feos_torch_amd import GcPcSaftMix

    tab = gp.table()
    cols = [torch.tensor([v[k] for _, v in tab], dtype=f64, requires_grad=grad) for k in range(8)]
    kab = torch.tensor([k[2] for k in c.kab_list], dtype=f64, requires_grad=grad)
    kl = [(k[0], k[1], kv) for k, kv in zip(c.kab_list, kab)]
    ph = torch.tensor(c.phi[idx], dtype=f64, device=device, requires_grad=grad)
    eos = GcPcSaftMix([s for s, _ in tab], tuple(cols), [c.segment_lists[i] for i in idx], [c.bond_lists[i] for i in idx], kl, ph)
    return eos, cols, kab, ph


def _run(g, idx, start, order=True, table=None, S=None, p_spec=None, t_init=None, z=None, phi=None):
    """pcs_gc_bubble_dew_temperature on the rows idx; order True: native.gc_class_order of these rows"""
    from feos_torch_amd import native

    c = g.c
    table, S = (g.table, g.S) if table is None else (table, S)
    rows = g.rows[_d(idx)].contiguous()
    od = native.gc_class_order(table, S, rows) if order is True else order
    r = native.gc_bubble_dew_temperature(table, S, rows, _d(c.phi[idx] if phi is None else phi),
                                         _d(c.p_spec[idx] if p_spec is None else p_spec), _d(c.z[idx] if z is None else z),
                                         _d(start * c.T[idx] if t_init is None else t_init), g.dew, want_iters=True, order=od)
    return {k: v.cpu().numpy() for k, v in r.items()}


@pytest.fixture(scope="module")
def ctx(oracle, hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from feos_torch_amd import native

    out = {}
    for dew in PROBLEMS:
        c = ref.inputs(oracle, dew)
        g = Ctx()
        g.c, g.dew = c, dew
        eos = _model(c, np.arange(c.n))[0]
        g.table, g.S, g.rows = eos._table(), eos.S, eos.rows
        # the existing pressure kernel at T_grid and at the displaced starts: e, and the must-solve set
        solved = c.keep.copy()
        for s in ref.STARTS:
            r = native.gc_bubble_dew(g.table, g.S, g.rows, _d(c.phi), _d(s * c.T), _d(c.z), _d(c.p_spec), dew,
                                     order=native.gc_class_order(g.table, g.S, g.rows))
            st = r["status"].cpu().numpy()
            solved &= ~st
            if s == 1.0:
                p_gpu, st_grid = r["p"].cpu().numpy(), st
        g.must = solved
        share = {int(k): float(np.mean(g.must[c.cell == k])) for k in c.cells}
        assert min(share.values()) >= 0.90, share  # before the new kernel is looked at
        g.e = ref.per_cell_max(c, _rel(p_gpu, c.p_spec), c.keep & ~st_grid)
        g.bar = np.maximum(1e-10, 10.0 * g.e)
        g.bar_rho = np.maximum(1e-10, g.bar * ref.per_cell_max(c, c.dlnrho_dlnp, c.keep))
        g.perm = ref.interleave(c.n)
        g.inv = np.argsort(g.perm)
        g.runs = {}
        for order in ORDERS:
            idx = g.perm if order == "interleaved" else np.arange(c.n)
            back = g.inv if order == "interleaved" else np.arange(c.n)
            for s in ref.STARTS:
                g.runs[order, s] = {key: v[back] for key, v in _run(g, idx, s).items()}
        print("%-7s must-solve %d of %d rows (oracle keeps %d); e = %.2e (largest cell), bar_T <= %.2e, bar_rho <= %.2e" % (
            name(dew), g.must.sum(), c.n, c.keep.sum(), g.e.max(), g.bar.max(), g.bar_rho.max()))
        out[dew] = g
    return out


@pytest.mark.parametrize("dew", PROBLEMS)
def test_values_against_the_long_double_oracle(ctx, dew):
    g = ctx[dew]
    c = g.c
    for key, r in g.runs.items():
        ok = c.keep & ~r["status"]
        eT = _rel(r["t"], c.T)
        er = _rel(r["rho4"], c.rho4).max(axis=1)
        print("%-7s %-12s start %.2f  solved %4d / %4d kept  T %.2e  rho4 %.2e  trials: median %d, max %d" % (
            name(dew), key[0], key[1], ok.sum(), c.keep.sum(), eT[ok].max(), er[ok].max(), np.median(r["iters"][ok]), r["iters"][ok].max()))
        assert (eT[ok] <= g.bar[ok]).all(), (key, np.nonzero(ok & (eT > g.bar))[0], eT[ok].max())
        assert (er[ok] <= g.bar_rho[ok]).all(), (key, np.nonzero(ok & (er > g.bar_rho))[0], er[ok].max())


@pytest.mark.parametrize("dew", PROBLEMS)
def test_every_must_solve_row_is_solved_from_all_three_starts(ctx, dew):
    g = ctx[dew]
    for key, r in g.runs.items():
        missed = np.nonzero(g.must & r["status"])[0]
        assert len(missed) == 0, (key, missed)
        bad = r["status"]
        assert (r["iters"][bad] == -1).all() and (r["t"][bad] == 0).all() and (r["rho4"][bad] == 0).all()
        assert (r["iters"][~bad] >= 1).all()


@pytest.mark.parametrize("dew", PROBLEMS)
def test_bad_inputs_are_flagged_and_wave_mates_unchanged(ctx, dew):
    g = ctx[dew]
    c = g.c
    n = 384
    idx = np.arange(n)
    bad = (0.0, -1.0, float("nan"), float("inf"), float("-inf"))
    bad_z = bad + (1.0,)
    bad_phi = (-1.0, float("nan"), float("inf"), float("-inf"))
    p, t0, z, phi = c.p_spec[:n].copy(), 0.93 * c.T[:n], c.z[:n].copy(), c.phi[:n].copy()
    rows_p, rows_t = np.arange(3, 3 + 7 * len(bad), 7), np.arange(70, 70 + 11 * len(bad), 11)
    rows_z, rows_f = np.arange(130, 130 + 13 * len(bad_z), 13), np.arange(260, 260 + 17 * len(bad_phi), 17)
    p[rows_p], t0[rows_t], z[rows_z] = bad, bad, bad_z
    phi[rows_f, np.arange(len(bad_phi)) % 2] = bad_phi
    r = _run(g, idx, 0.93, p_spec=p, t_init=t0, z=z, phi=phi)
    clean = g.runs["as built", 0.93]
    planted = np.concatenate((rows_p, rows_t, rows_z, rows_f))
    assert len(np.unique(planted)) == len(planted)
    assert r["status"][planted].all(), planted[~r["status"][planted]]
    mates = np.ones(n, dtype=bool)
    mates[planted] = False
    for key in KEYS:
        assert np.array_equal(r[key][mates], clean[key][:n][mates]), key
    assert (r["t"][~mates] == 0).all() and (r["rho4"][~mates] == 0).all() and (r["iters"][~mates] == -1).all()


@pytest.mark.parametrize("dew", PROBLEMS)
def test_solved_rows_are_never_wrong(ctx, dew, oracle):
    g = ctx[dew]
    c = g.c
    for key, r in g.runs.items():
        if key[0] != "as built":
            continue  # the interleaved runs have the same bits (test_schedule_independence)
        ok = ~r["status"]
        assert np.isfinite(r["t"][ok]).all() and (r["t"][ok] > 0).all() and np.isfinite(r["rho4"][ok]).all()
        idx = np.nonzero(ok)[0]
        p, _, st = oracle.gc_bubble_dew(ref.sub_enc(c.enc, idx), c.phi[idx], r["t"][idx], c.z[idx], c.p_spec[idx], dew, prec=1)
        assert not st[c.keep[idx]].any()
        chk = idx[~st]
        err = _rel(p[~st], c.p_spec[chk])
        lim = np.maximum(15.0, np.where(np.isfinite(c.dlnp_dlnT[chk]), c.dlnp_dlnT[chk], 15.0)) * g.bar[chk]
        print("%-7s start %.2f  oracle p(T) vs p_spec: %.2e on %d rows (%d solved rows the oracle does not answer)" % (
            name(dew), key[1], err.max(), len(chk), st.sum()))
        assert (err <= lim).all(), (key, chk[err > lim])


@pytest.mark.parametrize("dew", PROBLEMS)
def test_schedule_independence(ctx, dew):
    from feos_torch_amd.gc_pcsaft import build_table

    g = ctx[dew]
    c = g.c
    for s in ref.STARTS:
        a, b = g.runs["as built", s], g.runs["interleaved", s]
        for key in KEYS:
            assert np.array_equal(a[key], b[key]), (s, key)
    full = g.runs["as built", 0.93]
    everything = np.arange(c.n)
    for n in PREFIXES:
        for order in (True, None):
            part = _run(g, everything[:n], 0.93, order=order)
            for key in KEYS:
                assert np.array_equal(part[key], full[key][:n]), (n, order, key)
    plain = _run(g, everything, 0.93, order=None)
    for key in KEYS:
        assert np.array_equal(plain[key], full[key]), key
    # the table padded with unused segment types to S = 32 (the largest table: the LDS of one workgroup must still fit)
    S = g.S
    assert S < 32
    seg = g.table[: S * 8].view(S, 8)
    kab = 1.0 - g.table[S * 8 + 2 * S * S:].view(S, S)
    seg32 = torch.cat((seg, seg[:1].repeat(32 - S, 1)))
    kab32 = torch.zeros((32, 32), dtype=f64, device=seg.device)
    kab32[:S, :S] = kab
    for order in (True, None):
        padded = _run(g, everything, 0.93, order=order, table=build_table(seg32, kab32), S=32)
        for key in KEYS:
            assert np.array_equal(padded[key], full[key]), (order, key)


@pytest.mark.parametrize("dew", PROBLEMS)
def test_start_independence(ctx, dew):
    g = ctx[dew]
    k = g.must
    base = g.runs["as built", 1.0]["t"]
    for s in ref.STARTS[1:]:
        d = _rel(g.runs["as built", s]["t"], base)
        print("%-7s start %.2f vs 1.00: %.2e" % (name(dew), s, d[k].max()))
        assert (d[k] <= 2.0 * g.bar[k]).all()


@pytest.mark.parametrize("dew", PROBLEMS)
def test_gradients_against_the_referee_quotient(ctx, dew, oracle):
    g = ctx[dew]
    c = g.c
    wt = ref.weighted(oracle, c, dew)
    # the bars, from the referee alone
    q, q64 = ref.quotient(c.grad_row), ref.quotient(c.grad_row64)
    with np.errstate(invalid="ignore", divide="ignore"):
        e_row = np.abs(q64 - q).max(axis=1) / np.abs(q).max(axis=1)
        e_p = np.abs(q64[:, 2] / q[:, 2] - 1.0)
    bar_row = np.maximum(1e-10, 10.0 * ref.per_cell_max(c, e_row, c.keep))
    bar_p = np.maximum(1e-10, 10.0 * ref.per_cell_max(c, e_p, c.keep))
    rowsd = {"enc": c.enc, "kab_list": c.kab_list}
    e_kab = gp.kab_error(rowsd, wt["kab64"], wt["grad_kab"])
    bar_kab = max(1e-10, 10.0 * e_kab)
    assert np.all(wt["seg_self_error"] < 1e-8), wt["seg_self_error"]
    bar_seg = np.maximum(1e-10, 10.0 * wt["seg_self_error"])

    eos, cols, kab, ph = _model(c, np.arange(c.n), grad=True)
    ps = c.p_spec.copy()
    ps[list(ref.DROPPED)] = -1.0
    p = torch.tensor(ps, dtype=f64, requires_grad=True)
    z, t0 = torch.tensor(c.z, dtype=f64, requires_grad=True), torch.tensor(0.93 * c.T, dtype=f64, requires_grad=True)
    T, nans = (eos.dew_temperature if dew else eos.bubble_temperature)(p, z, t0)
    nans = nans.numpy()
    assert nans[list(ref.DROPPED)].all() and not nans[g.must & (wt["g"] != 0)].any()
    assert eos.rows.shape[0] == T.shape[0] == c.n - nans.sum()
    (T * torch.from_numpy(wt["g"][~nans])).sum().backward()
    assert z.grad is None and t0.grad is None
    assert (ph.grad.numpy()[nans] == 0).all() and (p.grad.numpy()[nans] == 0).all(), "dropped rows must receive zero gradient"
    # phi and p per row (rows of weight 0 carry no gradient: kept rows only)
    k = c.keep & ~nans & (wt["g"] != 0)
    got = np.concatenate((ph.grad.numpy(), p.grad.numpy()[:, None]), axis=1)[k] / wt["g"][k, None]
    want = q[k]
    err = np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)
    err_p = np.abs(got[:, 2] / want[:, 2] - 1.0)
    print("%-7s phi, p per row: %.2e of the row's largest component (oracle fp64 vs exact %.2e); dT/dp %.2e (%.2e)" % (
        name(dew), err.max(), e_row[c.keep].max(), err_p.max(), e_p[c.keep].max()))
    assert (err <= bar_row[k]).all(), np.nonzero(k)[0][err > bar_row[k]]
    assert (err_p <= bar_p[k]).all(), np.nonzero(k)[0][err_p > bar_p[k]]
    assert (got[:, 2] > 0).all(), "dT/dp > 0"
    # the four k_ab records
    want_k = gp.kab_records(rowsd, wt["grad_kab"])
    ek = float(np.max(np.abs(kab.grad.numpy() - want_k)) / np.max(np.abs(want_k)))
    print("%-7s k_ab records: %.2e (bar %.2e, oracle fp64 vs exact %.2e)" % (name(dew), ek, bar_kab, e_kab))
    assert ek <= bar_kab
    # the segment table
    got_seg = torch.stack([col.grad for col in cols], dim=1).numpy()
    es, used = gp.seg_error(rowsd, got_seg, wt["grad_seg"], mask_rows=wt["w"] != 0.0)
    print("%-7s segment table, error (bar) per column: " % name(dew)
          + " ".join("-" if np.isnan(e) else "%.1e (%.1e)" % (e, b) for e, b in zip(es, bar_seg)))
    assert np.isfinite(got_seg).all() and np.all(got_seg[~used] == 0.0)
    assert all(np.isnan(e) or e <= b for e, b in zip(es, bar_seg)), (es, bar_seg)
    # once_differentiable: the gradient carries no graph, so a second backward raises
    eos2, cols2, _, _ = _model(c, np.arange(8), grad=True)
    T2, _ = (eos2.dew_temperature if dew else eos2.bubble_temperature)(torch.tensor(c.p_spec[:8]), torch.tensor(c.z[:8]), torch.tensor(c.T[:8]))
    (g1,) = torch.autograd.grad(T2.sum(), cols2[0], create_graph=True)
    assert not g1.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable|differentiate twice|does not require grad"):
        g1.sum().backward()


@pytest.mark.parametrize("dew", PROBLEMS)
def test_round_trip_through_the_pressure_solve(ctx, dew):
    g = ctx[dew]
    c = g.c
    idx = np.nonzero(g.must)[0]
    eos = _model(c, idx)[0]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    T, nans = (eos.dew_temperature if dew else eos.bubble_temperature)(t(c.p_spec[idx]), t(c.z[idx]), t(1.07 * c.T[idx]))
    assert not nans.any().item()
    p, nans2 = (eos.dew_point if dew else eos.bubble_point)(T, t(c.z[idx]), t(c.p_spec[idx]))
    assert not nans2.any().item()
    err = _rel(p.numpy(), c.p_spec[idx])
    print("%-7s round trip: %.2e" % (name(dew), err.max()))
    assert (err <= 15.0 * g.bar[idx]).all(), idx[err > 15.0 * g.bar[idx]]


@pytest.mark.parametrize("dew", PROBLEMS)
def test_shell_conventions(ctx, dew):
    from feos_torch_amd import native

    g = ctx[dew]
    c = g.c
    n = 96
    idx = np.arange(n)
    p = c.p_spec[:n].copy()
    p[[5, 50]] = -1.0  # two rows fail
    call = lambda eos, *a, **kw: (eos.dew_temperature if dew else eos.bubble_temperature)(*a, **kw)
    # device tensors in -> device tensors out; the model is reduced
    eos = _model(c, idx, device="cuda")[0]
    T, nans = call(eos, _d(p), _d(c.z[:n]), _d(c.T[:n]))
    assert T.is_cuda and nans.is_cuda and nans.dtype == torch.bool and nans.shape == (n,) and T.shape == (n - int(nans.sum()),)
    assert nans[5].item() and nans[50].item() and int(nans.sum()) == 2
    assert eos.rows.shape[0] == T.shape[0] and eos.phi.shape[0] == T.shape[0]
    # CPU tensors in -> CPU tensors out
    cpu = lambda x: torch.from_numpy(np.array(x))
    eos_c = _model(c, idx)[0]
    Tc, nc = call(eos_c, cpu(p), cpu(c.z[:n]), cpu(c.T[:n]))
    assert not Tc.is_cuda and not nc.is_cuda and torch.equal(Tc, T.cpu()) and torch.equal(nc, nans.cpu())
    # check_stability: same T and nans, stable = stability_analysis of the specified phase at the returned state
    eos_s = _model(c, idx, device="cuda")[0]
    Ts, ns, stable = call(eos_s, _d(p), _d(c.z[:n]), _d(c.T[:n]), check_stability=True)
    assert torch.equal(Ts, T) and torch.equal(ns, nans) and stable.dtype == torch.bool and stable.shape == T.shape
    keep = np.nonzero(~nans.cpu().numpy())[0]
    r = _run(g, keep, 1.0, p_spec=p[keep])
    assert np.array_equal(r["t"], T.cpu().numpy())
    feed = _d(r["rho4"][:, 0:2] if dew else r["rho4"][:, 2:4])
    want, _, _ = eos_s.stability_analysis(T, feed)  # eos_s is reduced to the kept rows
    assert torch.equal(stable, want)
    assert native.gc_bubble_dew_temperature(g.table, g.S, g.rows[:0], _d(c.phi[:0]), _d(p[:0]), _d(p[:0]), _d(p[:0]), dew)["t"].shape == (0,)
