"""GPU: the gc-PC-SAFT state functions and their backward pass beyond one workgroup.

`pcs_gc_derivatives` (k_gc_derivatives) and `pcs_gc_derivatives_vjp` (k_gc_segment_gradient<MODE = 1>) behind
GcPcSaftMix.derivatives / helmholtz_energy_density at ordinary vapour, liquid and compressed-liquid densities of the config-5
distribution (feos_torch_amd.synthetic.gc_batch: branched alkanes, alcohols, amines, aldehydes, formates, ketones, the
induced-association pseudo-segment, '>C<' with epsilon_k = 0), on batches of several tiles, against

  * the long-double referee of the oracle (gc_derivatives(prec=1), gc_derivatives_vjp_exact), which tests/test_oracle_gc.py
    ties to the unmodified reference's values and autograd, and
  * the kernels themselves on other batch splits, row orders, table sizes, chunkings and under hipGraph replay.

States: the rows of gc_batch solved by the oracle's long-double bubble-point solver; per converged row the vapour, the liquid
and the liquid compressed by 1.15, all at the row's temperature.  Upstream weights ga, gp, gmu ~ N(0,1), gv ~ 1e-3 N(0,1)
(tests/test_dilute_gpu.py).

Tolerances (none is new): forward (a, p, mu, v) = (1e-12, 1e-11, 1e-12, 1e-9) in the measures of
tests/test_mixn_gpu.py::test_random_rows_vs_oracle; gradients 1e-7 of the row's (per-row inputs), the column's (segment table)
or the compared entries' (k_ab) largest component, as tests/test_deriv_grad_gpu.py.  A forward row may exceed its tolerance by
10 x the error of the fp64 oracle (prec=0, robust=True) on the same row (the rule of
tests/test_mix_gpu.py::test_derivatives_random_rows / tests/test_dilute_gpu.py for rows on which the formulas as written cancel
in fp64); at most 10 % of the rows may need that."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
f64 = torch.float64
FWD_TOL = (1e-12, 1e-11, 1e-12, 1e-9)
GRAD_TOL = 1e-7
CUTS = [1, 63, 64, 65, 191, 192, 193, 255, 256, 257, 1000]


@pytest.fixture(scope="module")
def amd():
    assert torch.cuda.is_available()
    import feos_torch_amd

    return feos_torch_amd


@pytest.fixture(scope="module")
def table():
    from feos_torch_amd.synthetic import load_segment_table

    return load_segment_table(os.path.join(ROOT, "tests", "data", "sauer2014_hetero.json"))


def _solved(oracle, table, n, seed):
    """gc_batch(n, seed) rows on which the oracle's long-double bubble point converges, with their three states."""
    from feos_torch_amd.synthetic import gc_batch

    b = gc_batch(n, table, seed=seed)
    enc = oracle.gc_encode(table, b["segment_lists"], b["bond_lists"], b["kab_list"])
    _, rho4, st = oracle.gc_bubble_dew(enc, b["phi"], b["T"], b["x"], b["p_init"], False, prec=1)
    dropped = float(st.mean())
    assert dropped <= 0.03, dropped
    keep = np.nonzero(~st)[0]
    enc = dict(enc, counts=np.ascontiguousarray(enc["counts"][keep]), bonds=np.ascontiguousarray(enc["bonds"][keep]))
    liq = np.ascontiguousarray(rho4[keep, 2:4])
    return {"segs": [b["segment_lists"][k] for k in keep], "bonds": [b["bond_lists"][k] for k in keep], "kab_list": b["kab_list"],
            "pick": b["pick"][keep], "phi": np.ascontiguousarray(b["phi"][keep]), "T": np.ascontiguousarray(b["T"][keep]), "enc": enc,
            "states": {"vapour": np.ascontiguousarray(rho4[keep, 0:2]), "liquid": liq, "compressed": 1.15 * liq},
            "dropped": dropped, "m": len(keep)}


@pytest.fixture(scope="module")
def big(oracle, table):
    return _solved(oracle, table, 3000, 2031)


@pytest.fixture(scope="module")
def mid(oracle, table):
    return _solved(oracle, table, 700, 2032)


def _weights(m, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=m), rng.normal(size=m), rng.normal(size=(m, 2)), 1e-3 * rng.normal(size=(m, 2))


def _np(x):
    return x.detach().cpu().numpy()


def _errors(a, p, mu, v, A, Pp, MU, V, rho):
    return (np.abs(a - A) / np.maximum(np.abs(A), 1e-6), np.abs(p - Pp) / np.maximum(np.abs(Pp), rho.sum(axis=1)),
            (np.abs(mu - MU) / np.maximum(1.0, np.abs(MU))).max(axis=1), np.abs(v / V - 1.0).max(axis=1))


def test_forward_vs_long_double_oracle(amd, oracle, table, big):
    """3000 rows x (vapour, liquid, compressed liquid) through GcPcSaftMix.derivatives against gc_derivatives(prec=1);
    helmholtz_energy_density is a[:, None] bit for bit.

    Measured on an MI355X (seed 2031; the oracle dropped 0.0 % of the rows), worst (a, p, mu, v) per state:
      vapour     2.19e-14  4.36e-16  2.78e-15  6.88e-15
      liquid     1.57e-15  6.91e-14  8.94e-15  1.11e-15
      compressed 2.65e-15  8.82e-15  2.34e-13  8.88e-16
    against the tolerances (1e-12, 1e-11, 1e-12, 1e-9); the fp64 oracle itself is as far from the long-double values (up to
    2.2e-14, 1.0e-13, 2.2e-13, 1.0e-14).  No row needed the fp64-noise allowance (0 of 3000, cap 10 %)."""
    ident = [s for s, _ in table]
    par = tuple(torch.tensor([v[k] for _, v in table], dtype=f64) for k in range(8))
    eos = amd.GcPcSaftMix(ident, par, big["segs"], big["bonds"], big["kab_list"], torch.tensor(big["phi"], dtype=f64))
    T = torch.tensor(big["T"], dtype=f64)
    print(f"\n{big['m']} rows, oracle dropped {100 * big['dropped']:.2f} %")
    need = np.zeros(big["m"], dtype=bool)
    for name, rho in big["states"].items():
        den = torch.tensor(rho, dtype=f64)
        a, p, mu, v = eos.derivatives(T, den)
        h = eos.helmholtz_energy_density(T, den)
        assert h.shape == (big["m"], 1) and _same_bits(h.detach(), a.detach()[:, None])
        a, p, mu, v = _np(a), _np(p), _np(mu), _np(v)
        assert all(np.all(np.isfinite(x)) for x in (a, p, mu, v))
        exact = oracle.gc_derivatives(big["enc"], big["phi"], big["T"], rho, prec=1)
        errs = _errors(a, p, mu, v, *exact, rho)
        noise = _errors(*oracle.gc_derivatives(big["enc"], big["phi"], big["T"], rho, robust=True), *exact, rho)
        print(f"   {name:10s} a {errs[0].max():.2e} p {errs[1].max():.2e} mu {errs[2].max():.2e} v {errs[3].max():.2e}   "
              f"(fp64 oracle: {noise[0].max():.2e} {noise[1].max():.2e} {noise[2].max():.2e} {noise[3].max():.2e})")
        for e, nz, tol in zip(errs, noise, FWD_TOL):
            assert np.all(e <= tol + 10.0 * nz), (name, tol, float(e.max()))
            need |= ~(e < tol)
    print(f"   rows that needed the fp64-noise allowance: {need.sum()} of {big['m']} ({100 * need.mean():.2f} %)")
    assert need.mean() <= 0.10


def test_backward_vs_exact_gradient(amd, oracle, table, mid):
    """700 rows (2 x 256 + 188: three tiles of the VJP kernel at BLOCK = 256, the last one ragged) x 3 states through autograd with
    every input requiring a gradient, against gc_derivatives_vjp_exact: the [S,8] segment table by column scale, the four k_ab
    records, phi, T and rho per row; everything finite, the '>C<' entries included.

    Measured on an MI355X (seed 2032, no row dropped), worst relative error per state (segment table, k_ab, phi, T, rho):
      vapour     6.53e-11  5.65e-16  5.59e-14  1.72e-12  5.33e-14
      liquid     1.76e-11  1.11e-15  1.06e-15  6.32e-14  2.73e-14
      compressed 4.36e-11  4.01e-16  2.51e-15  1.15e-13  5.20e-14
    against 1e-7 (the segment-table figure is the referee's finite differences, not the kernel); no noise allowance is applied
    to the gradients."""
    m = mid["m"]
    assert 2 * 256 < m <= 3 * 256 and m % 256 != 0, m
    ident = [s for s, _ in table]
    seg = mid["enc"]["seg"]
    used = mid["enc"]["counts"].sum(axis=(0, 1)) > 0
    assert used[ident.index(">C<")] and seg[ident.index(">C<"), 2] == 0.0
    for si, (name, rho) in enumerate(mid["states"].items()):
        ga, gp, gmu, gv = _weights(m, 11 + si)
        cols = [torch.tensor([v[k] for _, v in table], dtype=f64, requires_grad=True) for k in range(8)]
        kab = torch.tensor([k[2] for k in mid["kab_list"]], dtype=f64, requires_grad=True)
        kl = [(k[0], k[1], kv) for k, kv in zip(mid["kab_list"], kab)]
        ph = torch.tensor(mid["phi"], dtype=f64, requires_grad=True)
        T = torch.tensor(mid["T"], dtype=f64, requires_grad=True)
        den = torch.tensor(rho, dtype=f64, requires_grad=True)
        a, p, mu, v = amd.GcPcSaftMix(ident, tuple(cols), mid["segs"], mid["bonds"], kl, ph).derivatives(T, den)
        t = lambda x: torch.tensor(x, dtype=f64).to(a.device)
        ((a * t(ga)).sum() + (p * t(gp)).sum() + (mu * t(gmu)).sum() + (v * t(gv)).sum()).backward()
        gseg = np.stack([_np(c.grad) for c in cols], axis=1)  # [S,8]
        got_row = np.concatenate([_np(ph.grad), _np(T.grad)[:, None], _np(den.grad)], axis=1)
        gk = _np(kab.grad)
        assert np.all(np.isfinite(gseg)) and np.all(np.isfinite(got_row)) and np.all(np.isfinite(gk))
        grow, eseg, ekab = oracle.gc_derivatives_vjp_exact(mid["enc"], mid["phi"], mid["T"], rho, ga, gp, gmu, gv)
        worst = []
        e_seg = 0.0
        for k in range(8):
            mask = used & (seg[:, k] != 0.0)  # what the referee reports; the rest is 0 there and not compared
            assert mask.any() and np.all(eseg[~mask, k] == 0.0)
            e_seg = max(e_seg, float(np.max(np.abs(gseg[mask, k] - eseg[mask, k])) / np.max(np.abs(eseg[mask, k]))))
        assert np.all(gseg[~used] == 0.0)
        worst.append(e_seg)
        ek = np.array([ekab[ident.index(k[0]), ident.index(k[1])] for k in mid["kab_list"]])
        assert np.all(ek != 0.0)
        worst.append(float(np.max(np.abs(gk - ek)) / np.max(np.abs(ek))))
        for sl in (slice(0, 2), slice(2, 3), slice(3, 5)):
            scale = np.max(np.abs(grow[:, sl]), axis=1)
            worst.append(float(np.max(np.max(np.abs(got_row[:, sl] - grow[:, sl]), axis=1) / np.maximum(scale, 1e-300))))
        print(f"\n   {name:10s} segment table {worst[0]:.2e} k_ab {worst[1]:.2e} phi {worst[2]:.2e} T {worst[3]:.2e} rho {worst[4]:.2e}")
        assert max(worst) < GRAD_TOL, (name, worst)


# ---------------------------------------------------------------------------------------------------------------------------
# C-ABI level: the kernels against themselves
# ---------------------------------------------------------------------------------------------------------------------------
_INT_OF_SIZE = {1: torch.uint8, 4: torch.int32, 8: torch.int64}


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and torch.equal(a.view(_INT_OF_SIZE[a.element_size()]), b.view(_INT_OF_SIZE[b.element_size()]))


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


def _batch(tab, src, idx, rho, dev, seed):
    """Device arrays of the rows idx of a solved set with densities rho [len(idx), 2] and seeded upstream weights."""
    from feos_torch_amd.gc_pcsaft import encode_rows

    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    t, S = _device_table(tab, src["kab_list"], dev)
    uniq = np.unique(idx)
    enc = encode_rows([s for s, _ in tab], [src["segs"][k] for k in uniq], [src["bonds"][k] for k in uniq])
    rows = d(enc[np.searchsorted(uniq, idx)])
    ga, gp, gmu, gv = _weights(len(idx), seed)
    return {"table": t, "S": S, "rows": rows, "phi": d(src["phi"][idx]), "T": d(src["T"][idx]), "rho": d(rho), "n": len(idx),
            "g": (d(ga), d(gp), d(gmu), d(gv))}


def _fwd(native, b, sl=slice(None)):
    return native.gc_derivatives(b["table"], b["S"], b["rows"][sl], b["phi"][sl], b["T"][sl], b["rho"][sl])


def _vjp(native, b, sl=slice(None), g=None, order=None):
    g = tuple(x[sl] for x in b["g"]) if g is None else g
    return native.gc_derivatives_vjp(b["table"], b["S"], b["rows"][sl], b["phi"][sl], b["T"][sl], b["rho"][sl], *g, order=order)


def _col_err(got, want, scale_of=None):
    """largest |got - want| of an [S,8] gradient relative to the largest entry of the same parameter column"""
    scale = (want if scale_of is None else scale_of).abs().max(dim=0).values.clamp_min(1e-300)
    return float(((got - want).abs() / scale).max())


@pytest.fixture(scope="module")
def thousand(amd, table, big):
    """1000 rows of the 3000-row set, the three states in turn (row i is in state i % 3)."""
    idx = np.arange(1000)
    st = list(big["states"].values())
    rho = np.stack([st[i % 3][i] for i in idx])
    return _batch(table, big, idx, rho, torch.device("cuda:0"), seed=21)


def test_per_row_outputs_do_not_depend_on_batch_or_schedule(amd, thousand):
    """pcs_gc_derivatives / pcs_gc_derivatives_vjp on prefixes of a 1000-row batch (one lane, one wave +- 1, three waves +- 1,
    one 256-lane tile +- 1, four tiles): a, p, mu, v, jac9 and agg have the bits of the same rows inside the full batch; with
    the class order and with a random permutation as `order` they have the bits of the call without an order, and grad_seg
    agrees to 1e-12 of each column's largest entry (only the order of the atomic additions differs)."""
    from feos_torch_amd import native

    b = thousand
    full = (*_fwd(native, b), *_vjp(native, b)[1:])
    assert all(bool(torch.isfinite(x).all()) for x in full)
    for n in CUTS:
        sl = slice(0, n)
        part = (*_fwd(native, b, sl), *_vjp(native, b, sl)[1:])
        for k, (x, y) in enumerate(zip(part, full)):
            assert _same_bits(x, y[:n]), (n, k)
        gseg, jac9, agg = _vjp(native, b, sl)
        gen = torch.Generator().manual_seed(n)
        orders = {"class": native.gc_class_order(b["table"], b["S"], b["rows"][sl]),
                  "random": torch.randperm(n, generator=gen).to(torch.int32).to(b["rows"].device)}
        for name, order in orders.items():
            assert order.shape == (n,) and order.dtype == torch.int32
            go, jo, ao = _vjp(native, b, sl, order=order)
            assert _same_bits(jo, jac9) and _same_bits(ao, agg), (n, name)
            assert _col_err(go, gseg) < 1e-12, (n, name, _col_err(go, gseg))


def test_segment_gradient_is_additive_over_batch_splits(amd, thousand):
    """grad_seg(rows[:n]) + grad_seg(rows[n:1000]) = grad_seg(rows[:1000]) to 1e-12 of the column scale at every cut of
    the prefix test: a lane past the end of a batch that contributed (it repeats the last row) would break this at every cut
    that is no multiple of the tile.  Also: a second call into the same buffer doubles it, omitted upstream gradients are zero
    weights, and the VJP is linear in the upstream gradients."""
    from feos_torch_amd import native

    b = thousand
    whole, jac_whole, _ = _vjp(native, b)
    for n in CUTS[:-1]:
        head, tail = _vjp(native, b, slice(0, n))[0], _vjp(native, b, slice(n, 1000))[0]
        err = _col_err(head + tail, whole)
        assert err < 1e-12, (n, err)
    # accumulation: the ABI adds into grad_seg
    dev, n = b["rows"].device, b["n"]
    acc = torch.zeros((b["S"], 8), dtype=f64, device=dev)
    jac9, agg = torch.empty((n, 9), dtype=f64, device=dev), torch.empty((n, 6), dtype=f64, device=dev)
    for _ in range(2):
        native._call(dev, "pcs_gc_derivatives_vjp", b["table"], b["S"], b["rows"], b["phi"], b["T"], b["rho"], n, *b["g"], acc, jac9,
                     agg, None)
    assert _col_err(acc, 2.0 * whole, scale_of=whole) < 1e-12
    assert _same_bits(jac9, jac_whole)
    # omitted upstream gradients are zero weights; linearity in the upstream
    zeros = tuple(torch.zeros_like(x) for x in b["g"])
    sum_seg, sum_jac = torch.zeros_like(whole), torch.zeros_like(jac_whole)
    for k in range(4):
        only = tuple(x if j == k else None for j, x in enumerate(b["g"]))
        padded = tuple(x if j == k else z for j, (x, z) in enumerate(zip(b["g"], zeros)))
        g1, j1, _ = _vjp(native, b, g=only)
        g2, j2, _ = _vjp(native, b, g=padded)
        assert _same_bits(j1, j2), k
        assert _col_err(g1, g2) < 1e-12, k
        sum_seg += g1
        sum_jac += j1
    assert _col_err(sum_seg, whole) < 1e-12
    scale = jac_whole.abs().max(dim=1, keepdim=True).values.clamp_min(1e-300)
    assert float(((sum_jac - jac_whole).abs() / scale).max()) < 1e-12


PLAIN = {f"C{n}" for n in range(2, 11)} | {"isobutane", "neopentane", "isopentane", "acetone", "butanone", "2-propanol"} | \
        {f"C{n}OH" for n in range(2, 7)}


def test_table_size_selects_the_block_but_not_the_result(amd, table, big):
    """An alkane / alcohol / ketone sub-batch (up to 600 rows) forward and through the VJP on three tables: (a) the S = 6
    segments it uses, in file order, (b) the full table, S = 23, (c) the full table padded to S = 32 with renamed copies of
    existing segments that no molecule uses.

    Block size of k_gc_segment_gradient<1, BLOCK> (launch_gc_gradient<1>, GsBlock<1>): the workgroup needs
    8 * (8 S + 3 S^2 + 59 * BLOCK) + 64 S bytes of LDS (gc_lds_bytes with 48 + 11 doubles per thread, plus the [S,8]
    accumulator), and BLOCK is GsBlock<1> = 256, held to the 160 KB of a CU at S = 32 by a static_assert:
      S =  6: 122 464 B -> BLOCK 256;   S = 23: 138 416 B -> BLOCK 256;   S = 32: 149 504 B -> BLOCK 256.
    S = 32 is the largest table the ABI admits, so the VJP runs at BLOCK = 256 for EVERY table (its
    only instantiation), and no choice of S makes two different block sizes run.  (The bubble / dew gradient, MODE 0,
    needs 88 doubles per thread: there BLOCK = 256 never fits and BLOCK = 192 always does -- exactly 160 KB at S = 32;
    tests/test_gc_point_grad_gpu.py.)  What the three tables do change is the LDS layout (table stride S, offset of the
    accumulator, of the bond area and of the rows) and the segment indices.

    Forward outputs, jac9 and agg agree across the tables to 1e-12 relative (measured: bit-identical), the grad_seg rows of the
    shared segments to 1e-12 of the column scale (measured 1.3e-15), the rows of unused segments are exactly 0.0."""
    from feos_torch_amd import native
    from feos_torch_amd.synthetic import gc_molecule_library

    names = [m[0] for m in gc_molecule_library()]
    plain = np.array([n in PLAIN for n in names])
    idx = np.nonzero(plain[big["pick"]].all(axis=1))[0][:600]
    assert len(idx) >= 400, len(idx)
    used = sorted({s for k in idx for mol in big["segs"][k] for s in mol})
    assert set(used) == {"CH3", "CH2", ">CH", ">C<", "OH", ">C=O"}
    small = [(s, v) for s, v in table if s in used]
    padded = list(table) + [(f"pad{k}", table[k % len(table)][1].copy()) for k in range(32 - len(table))]
    assert (len(small), len(table), len(padded)) == (6, 23, 32)
    st = list(big["states"].values())
    rho = np.stack([st[j % 3][k] for j, k in enumerate(idx)])
    dev = torch.device("cuda:0")
    out = {}
    for name, tab in (("used", small), ("full", table), ("padded", padded)):
        b = _batch(tab, big, idx, rho, dev, seed=31)
        gseg, jac9, agg = _vjp(native, b)
        ident = [s for s, _ in tab]
        rest = [k for k, s in enumerate(ident) if s not in used]
        assert bool((gseg[rest] == 0.0).all()), name
        out[name] = (*_fwd(native, b), jac9, agg, gseg[[ident.index(s) for s in used]])
        assert all(bool(torch.isfinite(x).all()) for x in out[name])
    ref = out["full"]
    for name in ("used", "padded"):
        got = out[name]
        per_row = max(float(((x - y).abs() / y.abs().clamp_min(1e-300)).max()) for x, y in zip(got[:6], ref[:6]))
        e_seg = _col_err(got[6], ref[6])
        print(f"\n   table '{name}' vs full: per-row outputs {per_row:.2e}, grad_seg {e_seg:.2e}")
        assert per_row < 1e-12 and e_seg < 1e-12, (name, per_row, e_seg)


def _gradient_launch_constants():
    src = open(os.path.join(ROOT, "feos_torch_amd", "csrc", "gc_gradient.hip")).read()
    return tuple(int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) for name in ("GS_GRID", "GSBLOCK"))


def test_grid_stride_wraps(amd, oracle, table):
    """One batch of cap * BLOCK + 9001 rows, cap = GS_GRID * GSBLOCK / BLOCK = 512 workgroups of BLOCK = 256 lanes (the block of
    every table, see test_table_size_selects_the_block_but_not_the_result): 140 073 rows, so that the first 36 workgroups of the
    VJP's persistent grid run their loop a second time, the last of them on a ragged tile.  The rows are the liquid states of a
    2000-row solved set, repeated.  No oracle at this size: jac9 / agg and the forward outputs have the bits of the same rows
    evaluated in chunks of 50 000, and grad_seg equals the sum of the chunks' to 1e-11 of the column scale (the bound of
    tests/test_gc_gpu.py for this atomic reduction)."""
    from feos_torch_amd import native

    gs_grid, gsblock = _gradient_launch_constants()
    block = 256
    cap = gs_grid * gsblock // block
    n = cap * block + 9001
    assert (n + block - 1) // block > cap and n % block != 0
    src = _solved(oracle, table, 2000, 2033)
    idx = np.arange(n) % src["m"]
    b = _batch(table, src, idx, src["states"]["liquid"][idx], torch.device("cuda:0"), seed=41)
    gseg, jac9, agg = _vjp(native, b)
    fwd = _fwd(native, b)
    parts = torch.zeros_like(gseg)
    for lo in range(0, n, 50_000):
        sl = slice(lo, min(n, lo + 50_000))
        g, j, a = _vjp(native, b, sl)
        assert _same_bits(j, jac9[sl]) and _same_bits(a, agg[sl]), lo
        for x, y in zip(_fwd(native, b, sl), fwd):
            assert _same_bits(x, y[sl]), lo
        parts += g
    assert bool(torch.isfinite(gseg).all()) and bool(torch.isfinite(jac9).all())
    err = _col_err(gseg, parts)
    print(f"\n   {n} rows, grad_seg vs the sum over chunks: {err:.2e}")
    assert err < 1e-11, err


def test_hipgraph_replay_equals_eager(amd, oracle, table, big):
    """pcs_gc_derivatives and pcs_gc_derivatives_vjp on 20 000 rows captured in one hipGraph and replayed behind pending
    launches (the pattern of tests/test_gc_gpu.py::test_hipgraph_replay_of_solve_and_segment_gradient_equals_eager): per-row
    outputs bit-identical to the eager call, grad_seg to 1e-11 of its largest entry.  The zero fill of grad_seg is part of the
    capture: the second replay gives the same gradient, not twice it."""
    from feos_torch_amd import native

    n = 20_000
    dev = torch.device("cuda:0")
    idx = np.arange(n) % big["m"]
    st = list(big["states"].values())
    rho = np.stack([st[(i // big["m"]) % 3][i % big["m"]] for i in range(n)])
    b = _batch(table, big, idx, rho, dev, seed=51)
    ref = (*_fwd(native, b), *_vjp(native, b))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        _fwd(native, b)
        _vjp(native, b)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = (*_fwd(native, b), *_vjp(native, b))
    for rep in range(2):
        got[0].fill_(float("nan"))
        got[5].fill_(float("nan"))
        for _ in range(3):
            _fwd(native, b)
        graph.replay()
        torch.cuda.synchronize()
        for k in (0, 1, 2, 3, 5, 6):  # a, p, mu, v, jac9, agg
            assert _same_bits(got[k], ref[k]), (rep, k)
        assert bool(torch.isfinite(got[4]).all())
        assert (got[4] - ref[4]).abs().max() <= 1e-11 * ref[4].abs().max(), rep
