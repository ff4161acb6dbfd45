"""GPU: every gc-PC-SAFT kernel on molecules that fill all 8 segment and all 8 bond slots of the 80-byte row, with segment
indices up to 31 (rows of tests/tools/gc_full_rows.py; what the builders deliver is asserted in tests/test_gc_full_rows_cpu.py).
Until now every row of the suite came from synthetic.gc_molecule_library(): at most 4 segment types and 3 bond types per
molecule, no index above 22.

  a. state functions and their backward pass on heterogeneous full rows against the long-double oracle
     (bars of tests/test_gc_state_gpu.py)
  b. every gc entry point on aliased rows (alias table, S = 32) against the same rows as plain molecules (23-row table): an
     aliased molecule IS the plain molecule, the two runs differ by the order of their sums only
  c. bubble / dew points and their gradient kernels on heterogeneous full rows against the long-double oracle
     (bars of tests/test_gc_gpu.py, tests/test_gc_incipient_gpu.py, tests/test_gc_point_grad_gpu.py)
  d. GcPcSaftMix.bubble_point(incipient_molefracs=True) and liquid_density through autograd against the ABI calls (1e-12)

Bars of (b): max(1e-12, 10 x the fp64 ORACLE's own aliased-against-plain difference of the same quantity)
(gc_full_rows.alias_noise, held and printed by tests/test_gc_full_rows_cpu.py); 1e-12 of the scale is the bar the suite uses
for 'same rows, other table size or batch split', 10 its usual margin over a referee's own noise.  Where the oracle has no
fp64 twin of a quantity the nearest one stands in, named at each comparison in ALIAS_CALLS.

Batches are 700 rows: two 256-row tiles and a ragged one, three 192-row tiles and a ragged one.
Measured on an MI355X: see the tests' docstrings."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import gc_full_rows as fr  # noqa: E402
import gc_point_rows as gp  # noqa: E402

pytestmark = pytest.mark.gpu
f64 = torch.float64
FWD_TOL = (1e-12, 1e-11, 1e-12, 1e-9)  # tests/test_gc_state_gpu.py
GRAD_TOL = 1e-7
MODES = [("bubble", False), ("dew", True)]


@pytest.fixture(scope="module")
def amd(hip_lib):
    assert torch.cuda.is_available()
    import feos_torch_amd

    return feos_torch_amd


def _np(x):
    return x.detach().cpu().numpy()


def _d(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _device(rows):
    """device arrays of a row set of gc_full_rows, or of one of its solved sets with the set's table added"""
    from feos_torch_amd.gc_pcsaft import build_table, encode_rows

    tab = rows["table"]
    ident = [s for s, _ in tab]
    kab = torch.zeros((len(ident), len(ident)), dtype=f64)
    for s1, s2, k in rows["kab_list"]:
        kab[ident.index(s1), ident.index(s2)] = kab[ident.index(s2), ident.index(s1)] = k
    seg = torch.tensor(np.stack([v for _, v in tab]), dtype=f64)
    enc = encode_rows(ident, rows["segs"], rows["bonds"])
    return {"table": build_table(seg.cuda(), kab.cuda()), "S": len(ident), "rows": _d(enc), "enc": enc, "ident": ident,
            "phi": _d(rows["phi"]), "T": _d(rows["T"]), "x": _d(rows["x"]), "n": enc.shape[0]}


def _assert_full(enc, least):
    """the encoded bytes: rows in which BOTH molecules have 8 non-zero segment counts and 8 non-zero bond counts, ids up to 31"""
    full = (enc[:, 16:32] > 0).all(axis=1) & (enc[:, 64:80] > 0).all(axis=1)
    assert full.sum() >= least and enc[full, 0:16].max() == 31, (int(full.sum()), int(enc[:, 0:16].max()))
    return full


def _kab_sym(b, d01, d04):
    """[S,S] gradient w.r.t. the symmetric k_ab pairs from the per-row derivatives w.r.t. A01 and B01 (weights folded in)"""
    from feos_torch_amd.gc_pcsaft import _kab_gradient

    G = _kab_gradient(b["table"], b["S"], b["rows"], b["phi"], b["T"], d01.contiguous(), d04.contiguous())
    return G + G.t() - torch.diag(torch.diagonal(G))


def _col_err(got, want):
    scale = np.maximum(np.abs(want).max(axis=0), 1e-300)
    return float((np.abs(got - want) / scale).max())


# ---------------------------------------------------------------------------------------------------------------------------
# a. state functions on heterogeneous full rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hetero_state(oracle):
    rows = fr.hetero_rows()
    return rows, fr.encode(oracle, rows), fr.state_points(rows)


def test_state_functions_on_heterogeneous_full_rows(amd, oracle, hetero_state):
    """GcPcSaftMix.derivatives (pcs_gc_derivatives) on 700 rows over the ordered pairs of nine full molecules (8 / 8, perturbed
    pads: no two slots carry the same numbers) and four small ones, at T = 0.6 x the lower critical-temperature estimate, packing
    fractions 1e-3, 0.30, 0.42 of sum x_i sum n m sigma^3 and x = 0.3, 0.7, against gc_derivatives(prec=1): FWD_TOL with the
    '10 x the fp64 oracle's own error, at most 10 % of the rows' allowance of tests/test_gc_state_gpu.py.

    Measured on an MI355X (342 of the 700 rows have both molecules full): worst (a, p, mu, v) 1.11e-14 5.53e-14 4.25e-14 3.48e-12
    (the fp64 oracle itself: 1.14e-14 6.33e-14 7.35e-14 4.93e-12); no row needed the allowance."""
    rows, enc, rho = hetero_state
    b = _device(rows)
    full = _assert_full(b["enc"], 200)
    ident = b["ident"]
    par = tuple(torch.tensor([v[k] for _, v in rows["table"]], dtype=f64) for k in range(8))
    eos = amd.GcPcSaftMix(ident, par, rows["segs"], rows["bonds"], rows["kab_list"], torch.tensor(rows["phi"], dtype=f64))
    assert torch.equal(eos.rows.cpu(), torch.from_numpy(b["enc"]))
    got = tuple(_np(x) for x in eos.derivatives(torch.tensor(rows["T"], dtype=f64), torch.tensor(rho, dtype=f64)))
    assert all(np.all(np.isfinite(x)) for x in got)
    exact = oracle.gc_derivatives(enc, rows["phi"], rows["T"], rho, prec=1)
    errs = fr.state_errors(*got, *exact, rho)
    noise = fr.state_errors(*oracle.gc_derivatives(enc, rows["phi"], rows["T"], rho, robust=True), *exact, rho)
    print(f"\n   700 rows, {full.sum()} with both molecules full: a {errs[0].max():.2e} p {errs[1].max():.2e} mu {errs[2].max():.2e} "
          f"v {errs[3].max():.2e}   (fp64 oracle: " + " ".join(f"{e.max():.2e}" for e in noise) + ")")
    need = np.zeros(rows["n"], dtype=bool)
    for e, nz, tol in zip(errs, noise, FWD_TOL):
        assert np.all(e <= tol + 10.0 * nz), (tol, float(e.max()), int(np.argmax(e)))
        need |= ~(e < tol)
    print(f"   rows that needed the fp64-noise allowance: {need.sum()} of {rows['n']}")
    assert need.mean() <= 0.10


def test_backward_on_heterogeneous_full_rows(amd, oracle, hetero_state):
    """The same 700 state points through autograd with every input requiring a gradient (pcs_gc_derivatives_vjp: all 32 rows of
    the segment table, the 28 k_ab records of the variants, phi, T, rho) against gc_derivatives_vjp_exact at GRAD_TOL = 1e-7 in
    the measures of tests/test_gc_state_gpu.py; gradient rows of table segments no molecule uses are exactly 0.

    Measured on an MI355X: segment table 1.02e-08 (the referee's finite differences) k_ab 9.55e-13 phi 1.08e-12 T 1.09e-12
    rho 1.08e-12."""
    rows, enc, rho = hetero_state
    m, ident, seg = rows["n"], enc["ident"], enc["seg"]
    used = enc["counts"].sum(axis=(0, 1)) > 0
    assert used[23:].all() and not used.all()
    rng = np.random.default_rng(71)
    ga, gp_, gmu, gv = rng.normal(size=m), rng.normal(size=m), rng.normal(size=(m, 2)), 1e-3 * rng.normal(size=(m, 2))
    cols = [torch.tensor([v[k] for _, v in rows["table"]], dtype=f64, requires_grad=True) for k in range(8)]
    kab = torch.tensor([k[2] for k in rows["kab_list"]], dtype=f64, requires_grad=True)
    kl = [(k[0], k[1], kv) for k, kv in zip(rows["kab_list"], kab)]
    ph = torch.tensor(rows["phi"], dtype=f64, requires_grad=True)
    T = torch.tensor(rows["T"], dtype=f64, requires_grad=True)
    den = torch.tensor(rho, dtype=f64, requires_grad=True)
    a, p, mu, v = amd.GcPcSaftMix(ident, tuple(cols), rows["segs"], rows["bonds"], kl, ph).derivatives(T, den)
    t = lambda x: torch.tensor(x, dtype=f64).to(a.device)
    ((a * t(ga)).sum() + (p * t(gp_)).sum() + (mu * t(gmu)).sum() + (v * t(gv)).sum()).backward()
    gseg = np.stack([_np(c.grad) for c in cols], axis=1)
    got_row = np.concatenate([_np(ph.grad), _np(T.grad)[:, None], _np(den.grad)], axis=1)
    gk = _np(kab.grad)
    assert np.all(np.isfinite(gseg)) and np.all(np.isfinite(got_row)) and np.all(np.isfinite(gk))
    grow, eseg, ekab = oracle.gc_derivatives_vjp_exact(enc, rows["phi"], rows["T"], rho, ga, gp_, gmu, gv)
    worst = [0.0]
    for k in range(8):
        mask = used & (seg[:, k] != 0.0)
        assert mask.any() and np.all(eseg[~mask, k] == 0.0)
        worst[0] = max(worst[0], float(np.max(np.abs(gseg[mask, k] - eseg[mask, k])) / np.max(np.abs(eseg[mask, k]))))
    assert np.all(gseg[~used] == 0.0)
    ek = np.array([ekab[ident.index(k[0]), ident.index(k[1])] for k in rows["kab_list"]])
    assert (ek != 0.0).sum() >= 20 and np.all(gk[ek == 0.0] == 0.0)  # a record no row forms: plain CH=O is in no molecule
    worst.append(float(np.max(np.abs(gk - ek)) / np.max(np.abs(ek))))
    for sl in (slice(0, 2), slice(2, 3), slice(3, 5)):
        scale = np.max(np.abs(grow[:, sl]), axis=1)
        worst.append(float(np.max(np.max(np.abs(got_row[:, sl] - grow[:, sl]), axis=1) / np.maximum(scale, 1e-300))))
    print(f"\n   segment table {worst[0]:.2e} k_ab {worst[1]:.2e} phi {worst[2]:.2e} T {worst[3]:.2e} rho {worst[4]:.2e}")
    assert max(worst) < GRAD_TOL, worst


# ---------------------------------------------------------------------------------------------------------------------------
# b. alias equivalence of every entry point
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def alias_ctx(amd, oracle):
    """plain and aliased device rows with identical phi, T, x, the oracle's long-double solutions of the plain rows (bubble and
    dew: densities, pressures) and seeded weights"""
    ar = fr.alias_rows()
    out = {"plain": _device(ar["plain"]), "aliased": _device(ar["aliased"]), "noise": fr.alias_noise(oracle)}
    _assert_full(out["aliased"]["enc"], 100)
    assert out["plain"]["enc"][:, 0:16].max() < 23 and (out["plain"]["S"], out["aliased"]["S"]) == (23, 32)
    out["F"] = fr.fold_matrix(out["aliased"]["ident"], out["plain"]["ident"])
    for name, dew in MODES:
        s = fr.solved(oracle, ar["plain"], dew)
        assert s["m"] == 700
        out[name] = {"rho4": _d(s["rho4"]), "p": _d(s["p"]), "w": _d(s["w"])}
    out["rho"] = _d(fr.state_points(ar["plain"]))
    rng = np.random.default_rng(72)
    out["g"] = tuple(_d(x) for x in (rng.normal(size=700), rng.normal(size=700), rng.normal(size=(700, 2)), 1e-3 * rng.normal(size=(700, 2))))
    out["kab_list"] = ar["plain"]["kab_list"]
    return out


def _rel(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))) if got.size else 0.0


def _rows_err(got, want, groups):
    """per-row blocks: largest |got - want| of a column group over the largest |want| of that group in the row"""
    worst = 0.0
    for sl in groups:
        den = np.abs(want[:, sl]).max(axis=1)
        worst = max(worst, float((np.abs(got[:, sl] - want[:, sl]).max(axis=1) / np.where(den == 0.0, 1.0, den)).max()))
    return worst


JAC = (slice(0, 3), slice(3, 6), slice(6, 7))  # dp/d(A00, A01, A11), d(B00, B01, B11), dT
JAC9 = JAC + (slice(7, 9),)


def _fold_kab(c, G32):
    return fr.fold_records({"kab_list": c["kab_list"]}, G32, c["aliased"]["ident"])


def _records(c, G23):
    ident = c["plain"]["ident"]
    return np.array([G23[ident.index(s1), ident.index(s2)] for s1, s2, _ in c["kab_list"]])


def _run(native, c, which, call):
    """{output name: (kind, numpy array)} of one entry point on the plain ('plain') or the aliased rows"""
    b = c[which]
    args = (b["table"], b["S"], b["rows"], b["phi"])
    order = lambda: native.gc_class_order(b["table"], b["S"], b["rows"])
    fold_seg = (lambda G: c["F"] @ _np(G)) if which == "aliased" else _np
    fold_kab = (lambda G: _fold_kab(c, _np(G))) if which == "aliased" else (lambda G: _records(c, _np(G)))
    kind, _, mode = call.partition(":")
    dew = mode.startswith("dew")
    s = c["dew" if dew else "bubble"]
    if kind == "derivatives":
        a, p, mu, v = native.gc_derivatives(*args, b["T"], c["rho"])
        return {"state": ("state", tuple(_np(x) for x in (a, p, mu, v)))}
    if kind == "bubble_dew":
        r = native.gc_bubble_dew(*args, b["T"], b["x"], torch.full_like(b["T"], 1e5), dew, order=order() if mode.endswith("order") else None)
        return {"status": ("exact", _np(r["status"])), "p": ("p", _np(r["p"])), "rho4": ("rho4", _np(r["rho4"]))}
    if kind == "temperature":
        r = native.gc_bubble_dew_temperature(*args, s["p"], b["x"], 0.93 * b["T"], dew, order=order())
        return {"status": ("exact", _np(r["status"])), "t": ("p", _np(r["t"])), "rho4": ("rho4", _np(r["rho4"]))}
    if kind == "density":
        phase = int(mode.endswith("vapour"))
        r = native.gc_density(*args, b["T"], s["p"] * (0.5 if phase else 2.0), b["x"], phase, order=order())
        return {"status": ("exact", _np(r["status"])), "rho": ("rho4", _np(r["rho"])), "dpdrho": ("state_p", _np(r["dpdrho"]))}
    if kind == "stability":
        liq = s["rho4"][:, 2:4]
        scale = torch.where(torch.arange(b["n"], device=liq.device) % 2 == 0, 1.15, 0.3).to(f64)
        r = native.gc_stability(*args, b["T"], (liq * scale[:, None]).contiguous(), order=order())
        st, tpd = _np(r["status"]), _np(r["tpd"])
        done = np.isfinite(tpd)  # a row the search gives up on reports NaN
        return {"status": ("exact", st), "finite": ("exact", ~done), "tpd": ("tpd", np.where(done, tpd, 0.0)),
                "rho_trial": ("trial", (_np(r["rho_trial"]), (st != 0) & done))}
    if kind == "jacobian":
        jac, agg = native.gc_jacobian(*args, b["T"], s["rho4"], dew, order=order())
        jp, jy, agg2 = native.gc_point_jacobian(*args, b["T"], s["rho4"], dew, order=order())
        assert torch.equal(jp, jac) and torch.equal(agg, agg2)
        G = _kab_sym(b, s["w"] * jp[:, 1], s["w"] * jp[:, 4])
        Gy = _kab_sym(b, s["w"] * jy[:, 1], s["w"] * jy[:, 4])
        return {"jac_p": ("jac", _np(jp)), "jac_y": ("jac_y", _np(jy)), "agg": ("agg", _np(agg)), "k_ab of p": ("kab", fold_kab(G)),
                "k_ab of y": ("kab_y", fold_kab(Gy))}
    if kind == "segment_gradient":
        G = native.gc_segment_gradient(*args, b["T"], s["rho4"], dew, gout=s["w"], order=order())
        Gp = native.gc_point_segment_gradient(*args, b["T"], s["rho4"], dew, gout_p=s["w"], gout_y=None)
        Gy = native.gc_point_segment_gradient(*args, b["T"], s["rho4"], dew, gout_p=None, gout_y=s["w"])
        unused = {} if which == "plain" else {"unused": ("exact", _np(G)[~_used(b)])}
        return {"grad_seg": ("seg", fold_seg(G)), "grad_seg (point, p)": ("seg", fold_seg(Gp)), "grad_seg (point, y)": ("seg_y", fold_seg(Gy)),
                **unused}
    if kind == "derivatives_vjp":
        gseg, jac9, agg = native.gc_derivatives_vjp(*args, b["T"], c["rho"], *c["g"], order=order())
        G = _kab_sym(b, jac9[:, 1], jac9[:, 4])
        return {"grad_seg": ("seg_state", fold_seg(gseg)), "jac9": ("jac9", _np(jac9)), "agg": ("agg", _np(agg)), "k_ab": ("kab_state", fold_kab(G))}
    raise KeyError(call)


def _used(b):
    used = np.zeros(b["S"], dtype=bool)
    used[b["enc"][:, 0:16][b["enc"][:, 16:32] > 0]] = True
    return used


ALIAS_CALLS = ["derivatives", "bubble_dew:bubble", "bubble_dew:bubble,order", "bubble_dew:dew", "bubble_dew:dew,order",
               "temperature:bubble", "temperature:dew", "density:bubble,liquid", "density:dew,vapour", "stability:bubble",
               "jacobian:bubble", "jacobian:dew", "segment_gradient:bubble", "segment_gradient:dew", "derivatives_vjp"]


def test_aliased_rows_keep_their_classes(amd, alias_ctx):
    """native.gc_class_order gives a permutation of either encoding along which the class key (association class x polar) does
    not increase, and a row has the same class key as plain and as aliased molecules."""
    from feos_torch_amd import native

    cls = {}
    for which, tab in (("plain", fr.base_table()), ("aliased", fr.alias_table())):
        b = alias_ctx[which]
        o = _np(native.gc_class_order(b["table"], b["S"], b["rows"])).astype(int)
        assert sorted(o.tolist()) == list(range(b["n"]))
        counts, _ = fr.decode(b["enc"], b["S"])
        cls[which] = gp.class_key(np.stack([v for _, v in tab]), counts)
        assert np.all(np.diff(cls[which][o]) <= 0)
    assert np.array_equal(cls["plain"], cls["aliased"]) and len(set(cls["plain"].tolist())) == 6


@pytest.mark.parametrize("call", ALIAS_CALLS)
def test_aliased_rows_equal_plain_rows(amd, oracle, alias_ctx, call):
    """One entry point on the 700 aliased rows (S = 32; the six branched molecules at 8 / 8, C9 / C10 at 6 / 8, C6OH / C6NH2 at
    6 / 6, ids up to 31) and on the same rows as plain molecules (S = 23), identical phi, T, x, p: status bytes equal (the classes:
    test_aliased_rows_keep_their_classes),
    values and per-row Jacobian blocks equal, the segment-table gradient summed over the variants of a segment and the k_ab
    gradient summed over the variants of a record equal to the plain ones; gradient rows of unused table segments exactly 0.

    Bars max(1e-12, 10 x fp64 oracle, aliased against plain) with the oracle's figure for:  (a, p, mu, v) -> 'state';
    p, rho4 of the solver -> the oracle's fp64 solver; T of the temperature solve -> p (|d ln T / d ln p| < 1 below the critical
    point); density roots -> rho4, their dp/drho -> the state functions' p; tpd -> mu (a difference of chemical potentials, in
    units of max(1, |tpd|)), trial densities of unstable rows -> rho4; jac_p, agg -> dp/dphi, dp/dT of the exact gradient; k_ab
    of p -> its folded records; the segment table of p -> dp/dphi, dp/dT (the referee has no fp64 twin for the table).
    Everything of y (jac_y, its k_ab records and table gradient) -> v: the oracle has no dy/dtheta at all, and by the
    implicit-function theorem dy/dtheta = -(dF/drho)^-1 dF/dtheta with dF/drho made of dmu/drho and dp/drho, the second
    derivatives of the Helmholtz energy, of which v is the oracle's one output (v is also its noisiest: 1.5e-12).  The backward
    of the state functions (grad_seg, jac9, k_ab of derivatives_vjp) -> the largest of (a, p, mu, v): the functional is
    ga a + gp p + gmu mu + gv v.
    jac blocks per row and column group (A, B, T[, rho]) relative to the group's largest entry in the row.

    Measured on an MI355X (bar in brackets):
      derivatives        (a, p, mu, v) 2.3e-15 4.7e-14 1.7e-14 1.1e-12 (1.0e-12 1.0e-12 1.0e-12 1.5e-11)
      bubble_dew         bubble p 2.2e-14 (1.3e-12) rho4 4.0e-14 (1.8e-12); dew p 6.4e-14 (1.0e-12) rho4 6.4e-14 (2.4e-12); with the
                         class order the same figures
      temperature        bubble t 1.6e-15 (1.3e-12) rho4 1.1e-13 (1.8e-12); dew t 1.4e-15 (1.0e-12) rho4 6.0e-14 (2.4e-12)
      density            liquid rho 1.7e-15 (1.8e-12) dp/drho 7.8e-14 (1.0e-12); vapour rho 0 (2.4e-12) dp/drho 1.1e-16 (1.0e-12)
      jacobian           bubble jac_p 4.7e-15 jac_y 4.1e-12 agg 9.0e-16 k_ab of p 7.1e-16 k_ab of y 4.3e-16;
                         dew jac_p 3.1e-14 jac_y 2.2e-12 agg 9.0e-16 k_ab of p 1.2e-15 k_ab of y 2.1e-15 (1.0e-12; y 1.5e-11)
      segment_gradient   bubble 8.5e-15, point p 1.6e-14, point y 5.3e-13; dew 9.5e-15, 1.7e-14, 7.6e-14 (1.0e-12; y 1.5e-11)
      derivatives_vjp    grad_seg 1.2e-12 jac9 1.8e-12 agg 9.0e-16 k_ab 1.2e-12 (1.5e-11; agg 1.0e-12)
      stability          tpd 8.9e-15 (1.0e-12) trial densities of the unstable rows 2.8e-13 (1.8e-12)"""
    from feos_torch_amd import native

    c = alias_ctx
    nz = c["noise"]
    kind, _, mode = call.partition(":")
    pt = nz["dew" if mode.startswith("dew") else "bubble"]
    bars = {"p": fr.bar(pt["p"]), "rho4": fr.bar(pt["rho4"]), "state_p": fr.bar(nz["state"][1]), "tpd": fr.bar(nz["state"][2]),
            "trial": fr.bar(pt["rho4"]), "jac": fr.bar(max(pt["phi"], pt["T"])), "agg": fr.bar(max(pt["phi"], pt["T"])),
            "kab": fr.bar(pt["kab"]), "seg": fr.bar(max(pt["phi"], pt["T"])), "seg_state": fr.bar(nz["state"].max()),
            "jac9": fr.bar(nz["state"].max()), "kab_state": fr.bar(nz["state"].max()), "second": fr.bar(nz["state"][3])}
    want, got = _run(native, c, "plain", call), _run(native, c, "aliased", call)
    print(f"\n   {call}:", end="")
    failures = []
    for name, (what, w) in want.items():
        g = got[name][1]
        if what == "exact":
            assert np.array_equal(g, w), name
            assert not w.all(), name  # not every row failed
            continue
        if what == "state":
            err = [float(e.max()) for e in fr.state_errors(*g, *w, _np(c["rho"]))]
            bar = [fr.bar(x) for x in nz["state"]]
            print(" (a, p, mu, v) " + " ".join(f"{e:.1e}" for e in err) + " (bars " + " ".join(f"{x:.1e}" for x in bar) + ")", end="")
            failures += [(name, e, x) for e, x in zip(err, bar) if not e <= x]
            continue
        if what == "trial":
            (g, gm), (w, wm) = g, w
            assert np.array_equal(gm, wm) and wm.any() and not wm.all()
            err = _rel(g[wm], w[wm])
        elif what == "tpd":
            err = float(np.max(np.abs(g - w) / np.maximum(1.0, np.abs(w))))
        elif what in ("jac", "jac_y", "jac9"):
            err = _rows_err(g, w, JAC9 if what == "jac9" else JAC)
        elif what in ("seg", "seg_y", "seg_state"):
            err = _col_err(g, w)
        elif what in ("kab", "kab_y", "kab_state"):
            assert np.all(w != 0.0)
            err = float(np.max(np.abs(g - w)) / np.max(np.abs(w)))
        else:  # p, rho4, state_p, agg: relative, element by element, on rows that are solved
            ok = ~want["status"][1].astype(bool) if "status" in want else slice(None)
            assert np.all(np.isfinite(w[ok]))
            err = _rel(g[ok], w[ok])
        bar = bars["second" if what.endswith("_y") else what]
        print(f" {name} {err:.1e} ({bar:.1e})", end="")
        if not err <= bar:
            failures.append((name, err, bar))
    print()
    if "unused" in got:
        assert np.all(got["unused"][1] == 0.0)
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------------
# c. bubble / dew points and their gradients on heterogeneous full rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hetero_point(amd, oracle):
    out = {}
    rows = fr.hetero_rows()
    for name, dew in MODES:
        s = fr.solved(oracle, rows, dew)
        b = _device(dict(s, table=rows["table"]))
        _assert_full(b["enc"], 200)
        b["rho4"], b["w"] = _d(s["rho4"]), _d(s["w"])
        out[dew] = (s, b)
    return out


def _molefrac(rho4, dew):
    k = 2 if dew else 0
    return rho4[:, k] / (rho4[:, k] + rho4[:, k + 1])


@pytest.mark.parametrize("name,dew", MODES)
def test_points_on_heterogeneous_full_rows(amd, oracle, name, dew):
    """pcs_gc_bubble_dew (class order) on the 700 heterogeneous rows against the oracle's long-double solver, which keeps all of
    them: rows that disagree on the status below 1 % and failed rows below 3 % (tests/test_gc_gpu.py), p to 1e-9 and rho4 to 1e-8
    relative on the rows both solve (ibid.), the incipient mole fraction y to max(1e-10, max(1e-10, 10 e_p) max(1, |d ln y / d ln p|))
    per class (tests/test_gc_incipient_gpu.py; e_p = this run's pressure error in the class, the conditioning along T from two
    more long-double solves at T (1 +- 1e-4)).

    Measured on an MI355X, 700 rows each, no row failed: bubble p 4.02e-14 rho4 1.38e-13 y 9.41e-14 (bar <= 7.67e-10), y from
    2.3e-22 to 1; dew p 1.55e-13 rho4 1.68e-13 y 6.17e-14 (bar <= 1.13e-10), x from 5.1e-22 to 1."""
    from feos_torch_amd import native

    rows = fr.hetero_rows()
    enc = fr.encode(oracle, rows)
    b = _device(rows)
    full = _assert_full(b["enc"], 200)
    p, rho4, st = oracle.gc_bubble_dew(enc, rows["phi"], rows["T"], rows["x"], rows["p_init"], dew, prec=1)
    order = native.gc_class_order(b["table"], b["S"], b["rows"])
    r = native.gc_bubble_dew(b["table"], b["S"], b["rows"], b["phi"], b["T"], b["x"], _d(rows["p_init"]), dew, order=order)
    nn = _np(r["status"]).astype(bool)
    assert (nn != st).mean() < 0.01 and nn.mean() < 0.03, (float((nn != st).mean()), float(nn.mean()))
    both = ~nn & ~st
    assert both[full].sum() >= 200
    e_p = np.abs(_np(r["p"]) / p - 1.0)
    e_rho = np.abs(_np(r["rho4"]) / rho4 - 1.0).max(axis=1)
    ys = []
    for f in (1.0 - 1e-4, 1.0 + 1e-4):
        pf, rf, sf = oracle.gc_bubble_dew(enc, rows["phi"], f * rows["T"], rows["x"], rows["p_init"], dew, prec=1)
        both &= ~sf
        ys.append((np.log(np.where(sf, 1.0, _molefrac(rf, dew))), np.log(np.where(sf, 1.0, pf))))
    with np.errstate(invalid="ignore", divide="ignore"):
        cond = np.abs((ys[1][0] - ys[0][0]) / (ys[1][1] - ys[0][1]))
    y_want, y_got = _molefrac(rho4, dew), _molefrac(_np(r["rho4"]), dew)
    e_y = np.abs(y_got / y_want - 1.0)
    cls = fr.classes(oracle, rows)
    bar = np.full(rows["n"], 1e-10)
    for k in np.unique(cls):
        m = (cls == k) & both
        if m.any():
            bar[cls == k] = max(1e-10, max(1e-10, 10.0 * e_p[m].max()) * max(1.0, cond[m].max()))
    print(f"\n   {name}: {both.sum()} rows, GPU failed {nn.sum()}; p {e_p[both].max():.2e} rho4 {e_rho[both].max():.2e} "
          f"y {e_y[both].max():.2e} (bar <= {bar[both].max():.2e}); y in [{y_got[both].min():.3e}, {y_got[both].max():.17g}]")
    assert e_p[both].max() < 1e-9 and e_rho[both].max() < 1e-8
    assert (e_y[both] <= bar[both]).all(), np.nonzero(both & ~(e_y <= bar))[0]


@pytest.fixture(scope="module")
def hetero_referee(oracle):
    """{dew: {class name: long-double referee under w 1[class] with its fp64 twin}} (gc_point_rows.referee without 'all')"""
    out = {}
    for _, dew in MODES:
        s = fr.solved(oracle, fr.hetero_rows(), dew)
        out[dew] = {}
        for cname, w in gp.groups(s).items():
            if cname == "all":
                continue
            val, grow, gkab, gseg, err = oracle.gc_bubble_dew_vjp_exact(s["enc"], s["phi"], s["T"], s["rho4"], dew, w)
            _, row64, kab64, _, _ = oracle.gc_bubble_dew_vjp_exact(s["enc"], s["phi"], s["T"], s["rho4"], dew, w, prec=0, segments=False)
            out[dew][cname] = {"w": w, "grad_row": grow, "grad_kab": gkab, "grad_seg": gseg, "seg_self_error": err, "kab64": kab64,
                               "row64": row64}
    return out


@pytest.mark.parametrize("name,dew", MODES)
def test_point_gradients_on_heterogeneous_full_rows(amd, oracle, hetero_point, hetero_referee, name, dew):
    """pcs_gc_point_jacobian and pcs_gc_point_segment_gradient (gout_p = w 1[class]) at the oracle's densities of the 700
    heterogeneous rows against gc_bubble_dew_vjp_exact, class by class, at the bars of tests/test_gc_point_grad_gpu.py: phi and T
    per row and the k_ab records per class max(1e-10, 10 e), e = the referee's fp64 twin; the segment table per column and class
    max(1e-10, 10 seg_self_error); gradient rows of segments the class does not use exactly 0.

    Measured on an MI355X over the seven classes (none; none, polar; self; self, polar; induced, polar; cross; cross, polar):
    bubble phi <= 2.0e-15, T <= 2.6e-15, k_ab <= 4.8e-16 (bars 1e-10); table columns at most 0.13 of their bar (largest 3.1e-10
    against 3.3e-09, sigma of 'self'); dew phi <= 7.4e-15, T <= 1.7e-15, k_ab <= 2.0e-15; table at most 0.12 of the bar."""
    from feos_torch_amd import native
    from feos_torch_amd.gc_pcsaft import _phi_gradient

    s, b = hetero_point[dew]
    ref = hetero_referee[dew]
    jp, jy, agg = native.gc_point_jacobian(b["table"], b["S"], b["rows"], b["phi"], b["T"], b["rho4"], dew)
    got = np.concatenate([_np(_phi_gradient(jp, agg, b["phi"])), _np(jp[:, 6:7])], axis=1)
    assert np.isfinite(got).all() and bool(torch.isfinite(jy).all())
    print(f"\n   {name}")
    failures = []
    for cname, rf in ref.items():
        on = rf["w"] != 0.0
        bars = gp.row_bars({"row64": rf["row64"][on], "grad_row": rf["grad_row"][on]})
        err = gp.row_error(got[on], rf["grad_row"][on])
        for g, (e, bar) in bars.items():
            assert np.isfinite(e).all() and np.mean(bar > 1e-8) <= 0.05, (cname, g)
            if not (err[g] <= bar).all():
                failures.append((cname, g, float(err[g].max())))
        e = gp.kab_error(s, rf["kab64"], rf["grad_kab"])
        kbar = max(gp.FLOOR, 10.0 * e)
        wd = _d(rf["w"])
        got_k = _np(_kab_sym(b, wd * jp[:, 1], wd * jp[:, 4]))
        ek = gp.kab_error(s, got_k, rf["grad_kab"])
        want_rec = gp.kab_records(s, rf["grad_kab"])
        assert np.all(gp.kab_records(s, got_k)[want_rec == 0.0] == 0.0), cname
        assert np.all(rf["seg_self_error"] < 1e-8), (cname, rf["seg_self_error"])
        sbar = np.maximum(gp.FLOOR, 10.0 * rf["seg_self_error"])
        G = _np(native.gc_point_segment_gradient(b["table"], b["S"], b["rows"], b["phi"], b["T"], b["rho4"], dew, gout_p=wd, gout_y=None))
        assert np.isfinite(G).all()
        es, used = gp.seg_error(s, G, rf["grad_seg"], mask_rows=on)
        assert np.all(G[~used] == 0.0), cname
        print(f"      {cname:15s} phi {err['phi'].max():.1e} T {err['T'].max():.1e} k_ab {ek:.1e} ({kbar:.1e})  table "
              + " ".join("-" if np.isnan(x) else f"{x:.1e} ({y:.1e})" for x, y in zip(es, sbar)))
        if not ek <= kbar:
            failures.append((cname, "k_ab", ek, kbar))
        failures += [(cname, k, float(es[k]), float(sbar[k])) for k in range(8) if not np.isnan(es[k]) and not es[k] <= sbar[k]]
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------------
# d. through the API
# ---------------------------------------------------------------------------------------------------------------------------
def test_api_gradients_equal_the_abi_on_heterogeneous_full_rows(amd, oracle):
    """One GcPcSaftMix of the 700 heterogeneous rows with the eight parameter vectors, the 28 k_ab records and phi requiring
    gradients: bubble_point(incipient_molefracs=True) under random weights on p and y, then liquid_density at twice the bubble
    pressure under random weights.  Segment-table, k_ab and phi gradients equal the ABI calls on the kept rows
    (pcs_gc_point_jacobian + the host chains, pcs_gc_point_segment_gradient; pcs_gc_density + pcs_gc_derivatives_vjp) to 1e-12
    of the largest component (column, records, row): _kab_gradient scatters over all 8 id slots of both molecules here.

    Measured on an MI355X: bubble_point with y: k_ab 0, segment table 1.2e-14, phi 0; liquid_density: k_ab 0, table 2.0e-15, phi 0."""
    from feos_torch_amd import native
    from feos_torch_amd.gc_pcsaft import _GcDensity, _phi_gradient, build_table

    rows = fr.hetero_rows()
    ident = [s for s, _ in rows["table"]]
    n = rows["n"]

    def model():
        cols = [torch.tensor([v[k] for _, v in rows["table"]], dtype=f64, requires_grad=True) for k in range(8)]
        kab = torch.tensor([k[2] for k in rows["kab_list"]], dtype=f64, requires_grad=True)
        kl = [(k[0], k[1], kv) for k, kv in zip(rows["kab_list"], kab)]
        ph = torch.tensor(rows["phi"], dtype=f64, requires_grad=True)
        return amd.GcPcSaftMix(ident, tuple(cols), rows["segs"], rows["bonds"], kl, ph), cols, kab, ph

    def compare(cols, kab, ph, ok, Gseg, Gsym, gphi, what):
        want_k = torch.stack([Gsym[ident.index(k[0]), ident.index(k[1])] for k in rows["kab_list"]]).cpu()
        ek = float((kab.grad - want_k).abs().max() / want_k.abs().max())
        es = _col_err(np.stack([_np(c.grad) for c in cols], axis=1), _np(Gseg))
        gp_, wp = _np(ph.grad)[ok], _np(gphi)
        ep = float((np.abs(gp_ - wp).max(axis=1) / np.abs(wp).max(axis=1)).max())
        print(f"   {what}: k_ab {ek:.2e} segment table {es:.2e} phi {ep:.2e}")
        assert int((want_k != 0.0).sum()) >= 20 and bool((kab.grad[want_k == 0.0] == 0.0).all())  # plain CH=O is in no molecule
        assert max(ek, es, ep) < 1e-12, (what, ek, es, ep)
        assert np.all(_np(ph.grad)[~ok] == 0.0)

    T, x, p0 = (torch.tensor(rows[k], dtype=f64) for k in ("T", "x", "p_init"))
    rng = np.random.default_rng(73)
    print()
    # bubble point with the incipient composition
    eos, cols, kab, ph = model()
    rows0, dev = eos.rows.clone(), eos.rows.device
    _assert_full(_np(rows0), 200)
    p, nans, y = eos.bubble_point(T, x, p0, incipient_molefracs=True)
    ok = ~_np(nans).astype(bool)
    assert ok.mean() >= 0.97
    gp_w, gy_w = (torch.from_numpy(rng.uniform(0.5, 1.5, int(ok.sum()))) for _ in range(2))
    ((p * gp_w.to(p.device) * 1e-5).sum() + (y * gy_w.to(y.device)).sum()).backward()
    table = build_table(torch.stack([c.detach() for c in cols], dim=1).to(dev), eos.kab.detach().to(dev))
    sol = native.gc_bubble_dew(table, 32, rows0, ph.detach().to(dev), T.to(dev), x.to(dev), p0.to(dev), False,
                               order=native.gc_class_order(table, 32, rows0))
    assert np.array_equal(~_np(sol["status"]).astype(bool), ok)
    okd = torch.from_numpy(ok).to(dev)
    b = {"table": table, "S": 32, "rows": rows0[okd].contiguous(), "phi": ph.detach().to(dev)[okd].contiguous(), "T": T.to(dev)[okd].contiguous()}
    r4 = sol["rho4"][okd].contiguous()
    jp, jy, agg = native.gc_point_jacobian(table, 32, b["rows"], b["phi"], b["T"], r4, False)
    wp, wy = 1e-5 * gp_w.to(dev), gy_w.to(dev)
    block = wp[:, None] * jp + wy[:, None] * jy
    Gseg = native.gc_point_segment_gradient(table, 32, b["rows"], b["phi"], b["T"], r4, False, gout_p=wp, gout_y=wy)
    compare(cols, kab, ph, ok, Gseg, _kab_sym(b, block[:, 1], block[:, 4]), _phi_gradient(block, agg, b["phi"]), "bubble_point with y")
    # liquid density at twice the bubble pressure of the kept rows
    eos, cols, kab, ph = model()
    p_spec = torch.full((n,), 1e5, dtype=f64)
    p_spec[torch.from_numpy(ok)] = 2.0 * p.detach().cpu()
    rho, nans = eos.liquid_density(T, p_spec, x)
    ok = ~_np(nans).astype(bool)
    assert ok.mean() >= 0.97
    g = torch.from_numpy(rng.uniform(0.5, 1.5, int(ok.sum())))
    (rho * g.to(rho.device)).sum().backward()
    r = native.gc_density(table, 32, rows0, ph.detach().to(dev), T.to(dev), p_spec.to(dev), x.to(dev), 0, order=native.gc_class_order(table, 32, rows0))
    assert np.array_equal(~_np(r["status"]).astype(bool), ok)
    okd = torch.from_numpy(ok).to(dev)
    b = {"table": table, "S": 32, "rows": rows0[okd].contiguous(), "phi": ph.detach().to(dev)[okd].contiguous(), "T": T.to(dev)[okd].contiguous()}
    xk, rk = x.to(dev)[okd], r["rho"][okd]
    w = -(g.to(dev) * _GcDensity.C) / r["dpdrho"][okd]
    rho2 = torch.stack((xk * rk, (1.0 - xk) * rk), dim=1).contiguous()
    gseg, jac9, agg = native.gc_derivatives_vjp(table, 32, b["rows"], b["phi"], b["T"], rho2, g_p=w.contiguous())
    compare(cols, kab, ph, ok, gseg, _kab_sym(b, jac9[:, 1], jac9[:, 4]), _phi_gradient(jac9, agg, b["phi"]), "liquid_density")
