"""GPU: the two kernels behind the gradient of GcPcSaftMix.bubble_point / dew_point against an exact long-double referee, class
by class, and the launch geometry of the segment-gradient kernel's bubble / dew mode.

  pcs_gc_jacobian (k_gc_point_jacobian<true, false>)       jac [n,7] = dp/d(A00, A01, A11, B00, B01, B11, T), agg [n,6]; chained
                                                           to k_ab, phi and T by gc_pcsaft._kab_gradient / _phi_gradient
  pcs_gc_segment_gradient (k_gc_segment_gradient<0, 192>)  grad_seg [S,8] += sum_i g_i dp_i/d segment table

Referee: oracle.gc_bubble_dew_vjp_exact (DualN<long double, 4> for phi, T and every k_ab pair; Richardson-extrapolated
long-double central differences for the table), tied to the reference's autograd on the CPU by tests/test_oracle_gc.py.

Rows (tests/tools/gc_point_rows.py): gc_batch(720, seed=2041), all 720 rows converged by the oracle's long-double solver for
bubble and for dew = three tiles of 192 and a tail of 144.  Model classes of native.gc_class_order (association class x polar)
and their rows: none 97, none + polar 229, self 183, self + polar 126, induced + polar 15, cross 70.  Two classes cannot be
reached from gc_molecule_library: induced association needs the only molecule with acceptor sites alone, C3IA, whose 'IA' segment
carries a dipole, so every induced row is polar; cross association needs two of the alcohols and amines, none of which has a
polar segment, so no cross row is polar.  '>C<' (epsilon_k = 0) is used by 43 molecules.  A batch sum over these rows is
dominated by the first four classes; every comparison with the referee below is made once per class under the upstream
g = w 1[class], w ~ U(0.5, 1.5), besides once for the whole set.

Bars, all from the referee alone: max(1e-10, 10 e) with e = the referee's fp64 run against its long-double run (phi, T per row;
the four k_ab records per class sum), and per table column max(1e-10, 10 seg_self_error) with the referee's measured difference
between two Richardson extrapolations.  Measured on an MI355X: see the tests' docstrings.

Launch geometry of MODE 0 (launch_gc_gradient<0>, GsBlock<0>): the workgroup needs 24 S^2 + 128 S + 704 BLOCK bytes of LDS
(table 8 (8 S + 3 S^2), accumulator 64 S, and 16 + 61 + 11 = 88 doubles per thread).  BLOCK = 256 needs at least 180 224 B and never
fits the 163 840 B of a CU; BLOCK = 192 fits for every admissible S, so the tile is 192 rows for every table
(GsBlock<0>, held by a static_assert); at S = 32 the request is exactly 163 840 B, the whole LDS of a CU.  The persistent grid is capped at
GS_GRID * GSBLOCK / 192 = 682 workgroups, so the tile loop wraps above 130 944 rows.

Sensitivity, tried on a scratch build and not kept: see test_segment_gradient_vs_exact_gradient."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import gc_point_rows as gp  # noqa: E402

f64 = torch.float64
MODES = [("bubble", False), ("dew", True)]
CUTS = (1, 63, 64, 65, 191, 192, 193, 383, 384, 385)
PLAIN = {f"C{n}" for n in range(2, 11)} | {"isobutane", "neopentane", "isopentane", "acetone", "butanone", "2-propanol"} | \
        {f"C{n}OH" for n in range(2, 7)}


def test_row_set(oracle):
    """What the row set is for, from the oracle alone (no GPU): more than three 192-row tiles with a ragged tail, at most 3 % of
    the rows dropped by the oracle's solve (none is), every model class that gc_molecule_library can form -- worked out here from
    all 41 x 41 molecule pairs -- present with at least 8 rows, '>C<' in use."""
    from feos_torch_amd.synthetic import gc_molecule_library

    tab = gp.table()
    lib = gc_molecule_library()
    pairs = [(a, b) for a in range(len(lib)) for b in range(len(lib))]
    enc = oracle.gc_encode(tab, [[lib[a][1], lib[b][1]] for a, b in pairs], [[lib[a][2], lib[b][2]] for a, b in pairs], [])
    reachable = set(gp.class_key(enc["seg"], enc["counts"]).tolist())
    assert reachable == {0, 1, 2, 3, 5, 6}  # no non-polar induced, no polar cross association: see the module docstring
    print()
    for name, dew in MODES:
        r = gp.solved(oracle, dew)
        m = r["m"]
        assert r["dropped"] <= 0.03, r["dropped"]
        assert m > 3 * gp.TILE and m % gp.TILE != 0, m
        counts = {c: int((r["cls"] == c).sum()) for c in sorted(reachable)}
        print(f"   {name}: {m} rows ({m // gp.TILE} tiles + {m % gp.TILE}), dropped {100 * r['dropped']:.2f} %, "
              + ", ".join(f"{gp.CLASS_NAMES[c]} {k}" for c, k in counts.items()))
        assert all(k >= 8 for k in counts.values()), counts
        ident = r["enc"]["ident"]
        assert r["enc"]["counts"][:, :, ident.index(">C<")].sum() > 0 and r["enc"]["seg"][ident.index(">C<"), 2] == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def amd():
    assert torch.cuda.is_available()
    import feos_torch_amd

    return feos_torch_amd


def _np(x):
    return x.detach().cpu().numpy()


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64))


def _device_table(tab, kab_list, dev):
    """(flat device table, S) of a segment table [(identifier, array(8))] with the binary records that name its segments."""
    from feos_torch_amd.gc_pcsaft import build_table

    ident = [s for s, _ in tab]
    kab = torch.zeros((len(ident), len(ident)), dtype=f64)
    for s1, s2, k in kab_list:
        if s1 in ident and s2 in ident:
            kab[ident.index(s1), ident.index(s2)] = k
            kab[ident.index(s2), ident.index(s1)] = k
    seg = torch.tensor(np.stack([v for _, v in tab]), dtype=f64)
    return build_table(seg.to(dev), kab.to(dev)), len(ident)


def _device_rows(tab, r, idx=None):
    """Device arrays of the rows idx (default: all) of a solved set on the table tab: dict(table, S, rows, phi, T, rho4, x, w, n)."""
    from feos_torch_amd.gc_pcsaft import encode_rows

    dev = torch.device("cuda:0")
    idx = np.arange(r["m"]) if idx is None else np.asarray(idx)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    t, S = _device_table(tab, r["kab_list"], dev)
    uniq = np.unique(idx)
    enc = encode_rows([s for s, _ in tab], [r["segs"][k] for k in uniq], [r["bonds"][k] for k in uniq])
    return {"table": t, "S": S, "rows": d(enc[np.searchsorted(uniq, idx)]), "phi": d(r["phi"][idx]), "T": d(r["T"][idx]),
            "rho4": d(r["rho4"][idx]), "x": d(r["x"][idx]), "w": d(r["w"][idx]), "n": len(idx)}


@pytest.fixture(scope="module")
def dev_rows(amd, oracle):
    return {dew: _device_rows(gp.table(), gp.solved(oracle, dew)) for _, dew in MODES}


def _jac(native, b, dew, sl=slice(None), order=None):
    return native.gc_jacobian(b["table"], b["S"], b["rows"][sl], b["phi"][sl], b["T"][sl], b["rho4"][sl], dew, order=order)


def _seg(native, b, dew, sl=slice(None), gout=None, order=None):
    return native.gc_segment_gradient(b["table"], b["S"], b["rows"][sl], b["phi"][sl], b["T"][sl], b["rho4"][sl], dew,
                                      gout=gout, order=order)


def _kab(b, jac, g, sl=slice(None)):
    """[S,S] gradient w.r.t. the symmetric k_ab pairs under the upstream g: what autograd through the model's symmetric k_ab
    matrix hands the tensor of one binary record."""
    from feos_torch_amd.gc_pcsaft import _kab_gradient

    G = _kab_gradient(b["table"], b["S"], b["rows"][sl], b["phi"][sl], b["T"][sl], g * jac[:, 1], g * jac[:, 4])
    return G + G.t() - torch.diag(torch.diagonal(G))


def _col_err(got, want, scale_of=None):
    """largest |got - want| of an [S,8] gradient relative to the largest entry of the same parameter column"""
    scale = (want if scale_of is None else scale_of).abs().max(dim=0).values.clamp_min(1e-300)
    return float(((got - want).abs() / scale).max())


@pytest.mark.gpu
@pytest.mark.parametrize("name,dew", MODES)
def test_jacobian_vs_exact_gradient(amd, oracle, dev_rows, name, dew):
    """pcs_gc_jacobian at the oracle's densities, chained by _phi_gradient / _kab_gradient: dp/dphi (2) and dp/dT per row, the
    four k_ab records as the weighted sum of each class (and of the whole set), relative to the largest exact component of the
    group; bar max(1e-10, 10 e), e = the referee's fp64 run against its long-double run in the same measure.  From the referee
    alone: no row has a bar above 1e-8 (5 % allowed; largest e 1.2e-14).  With the class order as `order` jac and agg have the
    bits of the call without.

    Measured on an MI355X, largest error (every bar is the floor 1e-10; the referee's own e in brackets):
      bubble  phi 1.4e-15 (9.9e-15)  T 3.1e-15 (1.2e-14)  k_ab, worst class 3.4e-16 (none + polar; e at most 9.5e-16)
      dew     phi 1.2e-14 (1.3e-15)  T 1.8e-15 (1.5e-15)  k_ab, worst class 3.2e-15 (self; e at most 2.0e-16)"""
    from feos_torch_amd import native
    from feos_torch_amd.gc_pcsaft import _phi_gradient

    r, ref, b = gp.solved(oracle, dew), gp.referee(oracle, dew), dev_rows[dew]
    bars = gp.row_bars(ref["all"])
    for g, (e, bar) in bars.items():  # the bars hide nothing: from the referee alone, before the kernel is looked at
        assert np.isfinite(e).all() and np.mean(bar > 1e-8) <= 0.05, (g, float(np.mean(bar > 1e-8)))
    jac, agg = _jac(native, b, dew)
    order = native.gc_class_order(b["table"], b["S"], b["rows"])
    jo, ao = _jac(native, b, dew, order=order)
    assert jac.shape == (r["m"], 7) and agg.shape == (r["m"], 6)
    assert _same_bits(jo, jac) and _same_bits(ao, agg)
    got = np.concatenate([_np(_phi_gradient(jac, agg, b["phi"])), _np(jac[:, 6:7])], axis=1)
    assert np.isfinite(got).all()
    err = gp.row_error(got, ref["all"]["grad_row"])
    print(f"\n   {name}")
    for g, (e, bar) in bars.items():
        print(f"      {g:4s} per row   {err[g].max():.2e} ({np.max(err[g] / bar):.3f}; e {e.max():.2e})")
    for cname, w in gp.groups(r).items():
        e = gp.kab_error(r, ref[cname]["kab64"], ref[cname]["grad_kab"])
        bar = max(gp.FLOOR, 10.0 * e)
        got_k = _np(_kab(b, jac, torch.tensor(w, dtype=f64).to(jac.device)))
        ek = gp.kab_error(r, got_k, ref[cname]["grad_kab"])
        print(f"      k_ab {cname:15s} {ek:.2e} ({ek / bar:.3f}; e {e:.2e})")
        assert ek <= bar, (cname, ek, bar)
        want = gp.kab_records(r, ref[cname]["grad_kab"])
        assert np.all(gp.kab_records(r, got_k)[want == 0.0] == 0.0), cname  # a record no row of the class can form
    for g, (e, bar) in bars.items():
        assert (err[g] <= bar).all(), (g, int(np.argmax(err[g] / bar)), float(err[g].max()))


@pytest.mark.gpu
@pytest.mark.parametrize("name,dew", MODES)
def test_segment_gradient_vs_exact_gradient(amd, oracle, dev_rows, name, dew):
    """pcs_gc_segment_gradient once per class with gout = w 1[class] and once with all rows, against the referee under the same
    weights: every column scaled by the largest exact entry of that column FOR THAT CLASS, compared where the referee reports an
    entry, bar max(1e-10, 10 seg_self_error[k]) with the referee's own measured error of that call; the rows of segments the
    class does not use are exactly 0.

    Measured on an MI355X (every figure is of the size of the referee's own seg_self_error, a tenth of its bar; at most 0.14 of
    the bar; largest 1.4e-10, m of the induced + polar class, dew):
      bubble: error (bar) per column m, sigma, epsilon_k, mu, kappa_ab, epsilon_k_ab, na, nb
        all             1.5e-11 (2.2e-10) 5.1e-11 (7.3e-10) 4.8e-12 (1.0e-10) 1.5e-11 (1.3e-10) 7.4e-12 (1.0e-10) 8.7e-12 (1.3e-10) 2.0e-13 (1.0e-10) 1.7e-14 (1.0e-10)
        none            6.8e-12 (1.0e-10) 6.2e-11 (8.8e-10) 4.1e-12 (1.0e-10) - - - - -
        none, polar     1.3e-11 (1.7e-10) 6.1e-11 (8.8e-10) 3.6e-12 (1.0e-10) 1.5e-11 (1.3e-10) - - - -
        self            7.8e-12 (1.7e-10) 1.0e-10 (1.2e-09) 5.7e-12 (1.0e-10) - 7.6e-12 (1.3e-10) 2.3e-13 (1.0e-10) - -
        self, polar     7.6e-11 (1.0e-09) 1.2e-10 (1.7e-09) 6.6e-12 (1.0e-10) 1.5e-11 (1.3e-10) 5.3e-12 (1.1e-10) 1.4e-14 (1.0e-10) - -
        induced, polar  1.1e-10 (1.1e-09) 6.7e-11 (5.0e-10) 6.8e-12 (1.0e-10) 6.9e-12 (1.0e-10) 7.5e-12 (1.0e-10) 1.7e-11 (2.4e-10) 2.0e-13 (1.0e-10) 1.7e-14 (1.0e-10)
        cross           7.6e-11 (7.5e-10) 4.3e-11 (3.9e-10) 8.7e-12 (1.0e-10) - 9.8e-12 (1.1e-10) 1.5e-11 (2.2e-10) - -
      dew: error (bar) per column m, sigma, epsilon_k, mu, kappa_ab, epsilon_k_ab, na, nb
        all             7.9e-11 (9.6e-10) 1.3e-10 (1.8e-09) 7.9e-12 (1.0e-10) 9.6e-12 (1.0e-10) 3.6e-12 (1.0e-10) 5.3e-13 (1.0e-10) 4.1e-14 (1.0e-10) 2.4e-13 (1.0e-10)
        none            8.1e-12 (1.1e-10) 8.1e-11 (1.1e-09) 5.2e-12 (1.0e-10) - - - - -
        none, polar     6.9e-11 (9.6e-10) 1.2e-10 (1.7e-09) 7.7e-12 (1.0e-10) 9.6e-12 (1.0e-10) - - - -
        self            8.2e-11 (8.3e-10) 9.8e-11 (9.7e-10) 8.8e-12 (1.0e-10) - 5.6e-12 (1.1e-10) 1.2e-14 (1.0e-10) - -
        self, polar     1.2e-10 (1.4e-09) 5.6e-11 (6.2e-10) 6.9e-12 (1.0e-10) 8.0e-12 (1.0e-10) 2.8e-12 (1.0e-10) 5.8e-15 (1.0e-10) - -
        induced, polar  1.4e-10 (1.4e-09) 7.6e-11 (6.8e-10) 6.9e-12 (1.0e-10) 6.9e-12 (1.0e-10) 2.3e-12 (1.0e-10) 2.5e-12 (1.0e-10) 4.1e-14 (1.0e-10) 2.4e-13 (1.0e-10)
        cross           3.7e-11 (2.8e-10) 2.3e-11 (2.4e-10) 9.8e-12 (1.0e-10) - 3.1e-12 (1.0e-10) 2.0e-12 (1.0e-10) - -

    Sensitivity (scratch build, not kept): the ADJ_NA / ADJ_NB adjoints of the induced-association block, which only the 15
    induced + polar rows exercise, scaled by 1 + 1e-6 where gc_finish_gradient hands them on: this test reports 1.0e-6 in the na
    and nb columns of 'induced, polar' and of 'all' (bar 1e-10, 10^4 bars: red, bubble and dew).  tests/test_gc_seggrad_gpu.py goes
    red too on its four two-row autograd fixtures that hold an induced pair (1.0e-6 against 1e-7: no other class writes these two
    columns, so nothing dilutes them), while its 2000-row comparison with finite differences at 5e-6 stays green."""
    from feos_torch_amd import native

    r, ref, b = gp.solved(oracle, dew), gp.referee(oracle, dew), dev_rows[dew]
    print(f"\n   {name}: error (bar) per column m, sigma, epsilon_k, mu, kappa_ab, epsilon_k_ab, na, nb")
    failures = []
    for cname, w in gp.groups(r).items():
        assert np.all(ref[cname]["seg_self_error"] < 1e-8), (cname, ref[cname]["seg_self_error"])  # else: the referee's steps
        bar = np.maximum(gp.FLOOR, 10.0 * ref[cname]["seg_self_error"])
        got = _np(_seg(native, b, dew, gout=torch.tensor(w, dtype=f64).to(b["rows"].device)))
        assert np.isfinite(got).all()
        err, used = gp.seg_error(r, got, ref[cname]["grad_seg"], mask_rows=w != 0.0)
        assert np.all(got[~used] == 0.0), cname
        print(f"      {cname:15s} " + " ".join("        -        " if np.isnan(e) else f"{e:.1e} ({x:.1e})" for e, x in zip(err, bar)))
        for k in range(8):
            if not np.isnan(err[k]) and not err[k] <= bar[k]:
                failures.append((cname, k, float(err[k]), float(bar[k])))
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize("name,dew", MODES)
def test_shell_backward_equals_the_abi(amd, oracle, name, dew):
    """GcPcSaftMix.bubble_point / dew_point on the uncompacted 720-row batch with three rows made hopeless (T = NaN, -10 K,
    NaN phi), so that failed rows and native.Compaction are in the path; all eight segment vectors, the four k_ab, phi and T
    require a gradient, random upstream weights.  Segment and k_ab gradients equal the ABI calls on the kept rows to 1e-12 of the
    column / largest record (fp64 atomics and matrix products: order only); phi.grad and T.grad equal them bit for bit on the
    kept rows and are exactly 0 on the dropped ones."""
    from feos_torch_amd import native
    from feos_torch_amd.gc_pcsaft import _phi_gradient, build_table

    tab, bt = gp.table(), gp.batch()
    ident = [s for s, _ in tab]
    n = len(bt["T"])
    Tn, phin = bt["T"].copy(), bt["phi"].copy()
    Tn[100], Tn[333], phin[601, 0] = np.nan, -10.0, np.nan
    cols = [torch.tensor([v[k] for _, v in tab], dtype=f64, requires_grad=True) for k in range(8)]
    kab = torch.tensor([k[2] for k in bt["kab_list"]], dtype=f64, requires_grad=True)
    kl = [(k[0], k[1], kv) for k, kv in zip(bt["kab_list"], kab)]
    ph = torch.tensor(phin, dtype=f64, requires_grad=True)
    T = torch.tensor(Tn, dtype=f64, requires_grad=True)
    x, p0 = torch.tensor(bt["x"], dtype=f64), torch.tensor(bt["p_init"], dtype=f64)
    eos = amd.GcPcSaftMix(ident, tuple(cols), bt["segment_lists"], bt["bond_lists"], kl, ph)
    rows0, dev = eos.rows.clone(), eos.rows.device
    p, nans = (eos.dew_point if dew else eos.bubble_point)(T, x, p0)
    nans = nans.cpu()
    assert nans[[100, 333, 601]].all() and 3 <= int(nans.sum()) <= 0.03 * n
    ok = ~nans
    assert eos.rows.shape[0] == int(ok.sum()) == p.shape[0]  # the model was reduced: Compaction was in the path
    g = torch.from_numpy(np.random.default_rng(7 + int(dew)).uniform(0.5, 1.5, p.shape[0]))
    (p * g.to(p.device)).sum().backward()
    # the same through the C ABI on the kept rows
    table = build_table(torch.stack([c.detach() for c in cols], dim=1).to(dev), eos.kab.detach().to(dev))
    d = lambda v: v.detach().to(dev)
    sol = native.gc_bubble_dew(table, eos.S, rows0, d(ph), d(T), d(x), d(p0), dew, order=native.gc_class_order(table, eos.S, rows0))
    assert torch.equal(sol["status"].cpu(), nans)
    okd = ok.to(dev)
    rk, pk, Tk, r4, gd = rows0[okd].contiguous(), d(ph)[okd].contiguous(), d(T)[okd].contiguous(), sol["rho4"][okd].contiguous(), g.to(dev)
    assert _same_bits(sol["p"][okd], d(p))
    jac, agg = native.gc_jacobian(table, eos.S, rk, pk, Tk, r4, dew)
    want_phi = _phi_gradient(jac, agg, pk) * gd[:, None]
    want_T = gd * jac[:, 6]
    assert _same_bits(ph.grad[ok], want_phi.cpu()) and _same_bits(T.grad[ok], want_T.cpu())
    assert bool((ph.grad[nans] == 0.0).all()) and bool((T.grad[nans] == 0.0).all())
    bk = {"table": table, "S": eos.S, "rows": rk, "phi": pk, "T": Tk}
    Gk = _kab(bk, jac, gd).cpu()
    want_k = torch.stack([Gk[ident.index(k[0]), ident.index(k[1])] for k in bt["kab_list"]])
    ek = float((kab.grad - want_k).abs().max() / want_k.abs().max())
    want_seg = native.gc_segment_gradient(table, eos.S, rk, pk, Tk, r4, dew, gout=gd).cpu()
    got_seg = torch.stack([c.grad for c in cols], dim=1)
    es = _col_err(got_seg, want_seg)
    print(f"\n   {name}: {int(nans.sum())} rows dropped; shell against ABI: k_ab {ek:.2e}, segment table {es:.2e}")
    assert bool((want_k != 0.0).all()) and ek < 1e-12 and es < 1e-12, (ek, es)


@pytest.mark.gpu
@pytest.mark.parametrize("name,dew", MODES)
def test_mode0_tiles_of_192(amd, oracle, dev_rows, name, dew):
    """The tile of k_gc_segment_gradient<0, .> is 192 rows (module docstring), not the 256 of the Jacobian kernel at which
    tests/test_gc_seggrad_gpu.py cuts: grad(rows[:n]) + grad(rows[n:]) = grad(all 720) to 1e-12 of the column scale at n = one
    lane, one wave +- 1, one tile +- 1 and two tiles +- 1 (a lane past the end that contributed, or a wave of a ragged tile that
    was left out, breaks this), under the row weights of the set.  pcs_gc_jacobian on the prefixes, and at 255 / 256 / 257, has
    the bits of the whole call."""
    from feos_torch_amd import native

    b = dev_rows[dew]
    n_all = b["n"]
    whole = _seg(native, b, dew, gout=b["w"])
    jac, agg = _jac(native, b, dew)
    assert bool(torch.isfinite(whole).all()) and bool(torch.isfinite(jac).all())
    worst = 0.0
    for n in CUTS:
        assert 0 < n < n_all
        head = _seg(native, b, dew, slice(0, n), gout=b["w"][:n])
        tail = _seg(native, b, dew, slice(n, n_all), gout=b["w"][n:])
        err = _col_err(head + tail, whole)
        worst = max(worst, err)
        assert err < 1e-12, (n, err)
    for n in CUTS + (255, 256, 257):
        jn, an = _jac(native, b, dew, slice(0, n))
        assert jn.shape == (n, 7) and an.shape == (n, 6) and _same_bits(jn, jac[:n]) and _same_bits(an, agg[:n]), n
    print(f"\n   {name}: head + tail against the whole call, worst over the cuts {worst:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,dew", MODES)
def test_table_size_does_not_change_the_point_gradient(amd, oracle, name, dew):
    """The alkane / alcohol / ketone rows of the set (more than one tile) through pcs_gc_bubble_dew -> pcs_gc_jacobian ->
    pcs_gc_segment_gradient on the three tables of
    tests/test_gc_state_gpu.py::test_table_size_selects_the_block_but_not_the_result: (a) the S = 6 segments they use, (b) the
    full table, S = 23, (c) the full table padded to S = 32, the largest the ABI admits, with renamed copies no molecule uses.

    LDS of k_gc_segment_gradient<0, BLOCK>: 24 S^2 + 128 S + 704 BLOCK bytes.  BLOCK = 192 for every S (256 needs 180 224 B
    before the table): S = 6: 136 800 B, S = 23: 150 808 B, S = 32: 163 840 B -- exactly the LDS of a CU, accepted by the `<=`
    of the static_assert behind GsBlock and by the runtime.  k_gc_point_jacobian (BLOCK 256,24 S^2 + 64 S + 120 832 B) takes 147 456 B at S = 32;
    neither kernel nor the solver had run at S = 32.  What the tables change is the LDS layout and the segment indices, not the
    result: status is equal, p, rho4, jac and agg agree with the full table to 1e-12 relative, the grad_seg rows of the shared
    segments to 1e-12 of the column scale, and the rows of unused and padded segments are exactly 0.
    Measured on an MI355X (273 rows): per-row outputs bit-identical on all three tables, grad_seg to 3.3e-14."""
    from feos_torch_amd import native
    from feos_torch_amd.synthetic import gc_molecule_library

    r, table = gp.solved(oracle, dew), gp.table()
    names = [m[0] for m in gc_molecule_library()]
    plain = np.array([n in PLAIN for n in names])
    idx = np.nonzero(plain[r["pick"]].all(axis=1))[0]
    assert len(idx) > gp.TILE and len(idx) % gp.TILE != 0, len(idx)
    used = sorted({s for k in idx for mol in r["segs"][k] for s in mol})
    assert set(used) == {"CH3", "CH2", ">CH", ">C<", "OH", ">C=O"}
    small = [(s, v) for s, v in table if s in used]
    padded = list(table) + [(f"pad{k}", table[k % len(table)][1].copy()) for k in range(32 - len(table))]
    assert (len(small), len(table), len(padded)) == (6, 23, 32)
    out = {}
    for tname, tab in (("used", small), ("full", table), ("padded", padded)):
        b = _device_rows(tab, r, idx)
        p0 = torch.full((b["n"],), 1e5, dtype=f64, device=b["rows"].device)
        sol = native.gc_bubble_dew(b["table"], b["S"], b["rows"], b["phi"], b["T"], b["x"], p0, dew)
        ok = ~sol["status"]
        assert float(ok.double().mean()) >= 0.97, tname
        kept = {"table": b["table"], "S": b["S"], "n": int(ok.sum()), **{k: b[k][ok].contiguous() for k in ("rows", "phi", "T", "w")},
                "rho4": sol["rho4"][ok].contiguous()}
        jac, agg = _jac(native, kept, dew)
        gseg = _seg(native, kept, dew, gout=kept["w"])
        ident = [s for s, _ in tab]
        rest = [k for k, s in enumerate(ident) if s not in used]
        assert bool((gseg[rest] == 0.0).all()), tname
        out[tname] = (sol["status"], sol["p"][ok], sol["rho4"][ok], jac, agg, gseg[[ident.index(s) for s in used]])
        assert all(bool(torch.isfinite(v).all()) for v in out[tname][1:])
    ref = out["full"]
    msg = []
    for tname in ("used", "padded"):
        got = out[tname]
        assert torch.equal(got[0], ref[0]), tname
        per_row = max(float(((v - y).abs() / y.abs().clamp_min(1e-300)).max()) for v, y in zip(got[1:5], ref[1:5]))
        e_seg = _col_err(got[5], ref[5])
        msg.append(f"'{tname}' per-row outputs {per_row:.2e}, grad_seg {e_seg:.2e}")
        assert per_row < 1e-12 and e_seg < 1e-12, (tname, per_row, e_seg)
    print(f"\n   {name}: {len(idx)} rows; against the full table: " + "; ".join(msg))


def _gradient_launch_constants():
    src = open(os.path.join(ROOT, "feos_torch_amd", "csrc", "gc_gradient.hip")).read()
    return tuple(int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) for name in ("GS_GRID", "GSBLOCK"))


@pytest.mark.gpu
def test_mode0_grid_stride_wraps(amd, oracle):
    """One bubble-point batch of cap * 192 + 9001 rows, cap = GS_GRID * GSBLOCK / 192 = 682 workgroups: 139 945 rows, so that
    the first 47 workgroups of the persistent grid of k_gc_segment_gradient<0, 192> run their tile loop a second time, the last
    of them on a ragged tile.  The rows are the converged liquid / vapour pairs of a 2000-row solved set, repeated.  No oracle at
    this size: the whole call equals the sum over chunks of 50 000 rows to 1e-11 of the column scale (the bound of
    tests/test_gc_gpu.py for this atomic reduction), with and without the class order.
    Measured on an MI355X: 2.8e-15 without and 1.5e-15 with the class order."""
    from feos_torch_amd import native

    gs_grid, gsblock = _gradient_launch_constants()
    block = gp.TILE
    cap = gs_grid * gsblock // block
    n = cap * block + 9001
    assert cap == 682 and n == 139_945 and (n + block - 1) // block > cap and n % block != 0
    src = gp.solved(oracle, False, 2000, 2033)
    assert src["dropped"] <= 0.03
    b = _device_rows(gp.table(), src, np.arange(n) % src["m"])
    g = torch.from_numpy(np.random.default_rng(61).uniform(0.5, 1.5, n)).to(b["rows"].device)
    parts = torch.zeros((b["S"], 8), dtype=f64, device=b["rows"].device)
    for lo in range(0, n, 50_000):
        sl = slice(lo, min(n, lo + 50_000))
        parts += _seg(native, b, False, sl, gout=g[sl])
    errs = []
    for order in (None, native.gc_class_order(b["table"], b["S"], b["rows"])):
        whole = _seg(native, b, False, gout=g, order=order)
        assert bool(torch.isfinite(whole).all())
        errs.append(_col_err(whole, parts))
    print(f"\n   {n} rows, grad_seg against the sum over chunks: {errs[0]:.2e} without, {errs[1]:.2e} with the class order")
    assert max(errs) < 1e-11, errs
