"""GPU: tangent-plane stability analysis of binary feed states (pcs_mix_stability / pcs_gc_stability, PcSaftMix /
GcPcSaftMix.stability_analysis, bubble_point / dew_point(check_stability=True)) against hand cases and the brute-force CPU
referee (tests/tools/stability_referee.py, oracle only).

Feeds whose pressure the double-precision model does not determine to 1e-6 (stability_referee.mix_pressure_noise: a liquid
at ~1e-6 Pa, where the pressure is a difference of O(rho) terms and carries their rounding) are left out of the referee
comparison and counted: a vapour-like trial phase at such a pressure has an undetermined tpd (it moves by dp / p).  For the
same reason a returned trial phase is checked as a root of p = p^f to 1e-9 p^f plus that rounding (tests/test_stability_referee.py)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import stability_referee as R  # noqa: E402

pytestmark = pytest.mark.gpu
f64 = torch.float64
TPD_TOL = 1e-8


def _d(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _stab(P, K, T, rho):
    from feos_torch_amd import native

    r = native.mix_stability(_d(P), _d(K), _d(T), _d(rho))
    return r["status"].cpu().numpy(), r["tpd"].cpu().numpy(), r["rho_trial"].cpu().numpy()


def _reduced(p_pa, T):
    return p_pa / (1.380649e-23 * 1e30 * T)


def _pair(n, par, kij):
    return np.tile(np.asarray(par, dtype=np.float64), (n, 1, 1)), np.tile([kij, 0.0], (n, 1))


@pytest.fixture(scope="module")
def table():
    from feos_torch_amd.synthetic import load_segment_table

    return load_segment_table(os.path.join(ROOT, "tests", "data", "sauer2014_hetero.json"))


def test_identical_components_and_an_alkane_vapour(oracle):
    comp = [2.0, 3.5, 250.0, 0, 0, 0, 0, 0]
    T0 = 250.0
    psat, st = oracle.pure_vapor_pressure(np.array([comp]), np.array([T0]))
    assert not st.any()
    z = np.array([0.05, 0.3, 0.5, 0.8])
    n = len(z)
    P, K = _pair(n, [comp, comp], 0.0)
    T = np.full(n, T0)
    d, pk = R.mix_derivs(oracle, P, K, T), R.mix_packing(P, T)
    feeds = {}
    for name, fac, vap in (("compressed liquid", 3.0, False), ("vapour", 0.3, True), ("expanded liquid", 0.5, False)):
        rho = R.liquid_root(d, pk, z, np.full(n, _reduced(psat[0] * fac, T0)), vapour=vap)
        assert np.all(np.isfinite(rho)), name
        feeds[name] = np.stack([z * rho, (1 - z) * rho], axis=1)
    for name in ("compressed liquid", "vapour"):
        s, tpd, _ = _stab(P, K, T, feeds[name])
        print(name, s, tpd)
        assert np.all(s == 0) and np.all(tpd >= -1e-10), (name, s, tpd)
    s, tpd, tr = _stab(P, K, T, feeds["expanded liquid"])  # below the vapour pressure: metastable, the vapour is lower
    print("expanded liquid", s, tpd)
    assert np.all(s == 1) and np.all(tpd < -TPD_TOL)
    assert np.all(tr.sum(axis=1) < 0.1 * feeds["expanded liquid"].sum(axis=1))  # a vapour-like trial phase
    # n-pentane / n-hexane vapour at 300 K and 0.05 bar (both vapour pressures are above 0.2 bar)
    P, K = _pair(3, [[2.6896, 3.7729, 231.2, 0, 0, 0, 0, 0], [3.0576, 3.7983, 236.77, 0, 0, 0, 0, 0]], 0.0)
    T = np.full(3, 300.0)
    z = np.array([0.2, 0.5, 0.8])
    rho = R.liquid_root(R.mix_derivs(oracle, P, K, T), R.mix_packing(P, T), z, np.full(3, _reduced(5000.0, 300.0)), vapour=True)
    s, tpd, _ = _stab(P, K, T, np.stack([z * rho, (1 - z) * rho], axis=1))
    assert np.all(s == 0), (s, tpd)


def test_symmetric_liquid_liquid_split(oracle):
    """Two identical chain fluids with k_ij = 0.15 at 300 K, liquid at 10 bar (chosen with the referee on the CPU: binodal at
    z ~ 0.17 / 0.83, spinodal at ~ 0.29 / 0.71): status 0 outside the binodal, 1 between binodal and spinodal, 2 inside."""
    z = np.linspace(0.005, 0.995, 199)
    n = len(z)
    comp = [2.0, 3.5, 250.0, 0, 0, 0, 0, 0]
    P, K = _pair(n, [comp, comp], 0.15)
    T = np.full(n, 300.0)
    d, pk = R.mix_derivs(oracle, P, K, T), R.mix_packing(P, T)
    rho = R.liquid_root(d, pk, z, np.full(n, _reduced(10e5, 300.0)))
    feed = np.stack([z * rho, (1 - z) * rho], axis=1)
    ref = R.tpd_minimum(d, pk, feed)
    det = R.hessian_det(d, feed)  # spinodal from central differences of the oracle's mu
    want = np.where(det <= 0, 2, np.where(ref["tpd"] < -TPD_TOL, 1, 0))
    assert set(want.tolist()) == {0, 1, 2}
    print("binodal", z[want >= 1][[0, -1]], "spinodal", z[want == 2][[0, -1]])
    # points next to a boundary (within two grid steps) are not judged
    inner = np.ones(n, dtype=bool)
    for k in (1, 2):
        inner[k:] &= want[k:] == want[:-k]
        inner[:-k] &= want[:-k] == want[k:]
    s, tpd, tr = _stab(P, K, T, feed)
    assert np.array_equal(s[inner], want[inner]), (z[inner][s[inner] != want[inner]], s[inner][s[inner] != want[inner]])
    one = s == 1
    w = tr[one, 0] / tr[one].sum(axis=1)
    assert np.all((w - 0.5) * (z[one] - 0.5) < 0)  # the trial phase lies in the opposite lobe
    assert np.all(np.isneginf(tpd[s == 2])) and np.all(np.isnan(tr[s == 2]))


def test_invalid_feeds():
    P, K = _pair(5, [[2.0, 3.5, 250.0, 0, 0, 0, 0, 0], [1.5, 3.2, 200.0, 0, 0, 0, 0, 0]], 0.0)
    T = np.full(5, 250.0)
    rho = np.array([[0.0, 1e-3], [1e-3, -1e-4], [np.nan, 1e-3], [1e-3, np.inf], [1e-5, 1e-5]])
    s, tpd, tr = _stab(P, K, T, rho)
    assert np.all(s[:4] == 3) and np.all(np.isnan(tpd[:4])) and np.all(np.isnan(tr[:4]))
    assert s[4] == 0


def _converged_feeds(n, seed=78):
    from feos_torch_amd import native
    from feos_torch_amd.synthetic import mix_batch

    P, K, T, X, PI = mix_batch(n, seed=seed)
    out = {}
    for dew in (False, True):
        r = native.mix_bubble_dew(_d(P), _d(K), _d(T), _d(X), _d(PI), dew)
        ok = ~r["status"].cpu().numpy()
        rho4 = r["rho4"].cpu().numpy()
        out[dew] = (np.nonzero(ok)[0], rho4, r["p"].cpu().numpy())
    return (P, K, T, X, PI), out


def test_component_swap_symmetry(oracle):
    (P, K, T, X, PI), out = _converged_feeds(3000)
    for dew in (False, True):
        ok, rho4, _ = out[dew]
        feed = rho4[ok][:, 0:2] if dew else rho4[ok][:, 2:4]
        Pk, Kk, Tk = P[ok], K[ok], T[ok]
        s1, t1, r1 = _stab(Pk, Kk, Tk, feed)
        s2, t2, r2 = _stab(Pk[:, ::-1], Kk, Tk, feed[:, ::-1])
        # the tpd of a vapour-like trial at a dense feed moves with the relative rounding of p^f (~1e-16 sum(rho) / p^f), and
        # any tpd carries the rounding of the chemical potentials it is a difference of (|mu| ~ 45 at 1e-20 A^-3)
        _, pf, mu, _ = oracle.mix_derivatives(Pk, Kk, Tk, feed, robust=True)
        cond = feed.sum(axis=1) / np.abs(pf)
        mu_max = np.abs(np.log(feed) + mu).max(axis=1)
        judged = cond < 1e4
        fin = np.isfinite(t1) & np.isfinite(t2) & judged
        print(f"{'dew' if dew else 'bubble'}: {len(ok)} feeds, {judged.sum()} judged; status counts {np.bincount(s1, minlength=4)}")
        assert np.array_equal(s1[judged], s2[judged])
        assert np.array_equal(np.isinf(t1[judged]), np.isinf(t2[judged]))
        assert np.all(np.abs(t1[fin] - t2[fin]) <= 1e-12 + 1e-13 * cond[fin] + 4e-14 * mu_max[fin])
        both = (s1 == 1) & judged
        assert np.allclose(r1[both], r2[both][:, ::-1], rtol=1e-6, atol=0.0)


def _check_unstable(oracle, derivs, rows, P, K, T, feed, s, tpd, tr):
    """kernel status 1 -> an independent recomputation confirms the returned trial phase"""
    u = np.nonzero(s == 1)[0]
    if len(u) == 0:
        return
    noise = R.mix_pressure_noise(oracle, P[u], K[u], T[u], feed[u]) + R.mix_pressure_noise(oracle, P[u], K[u], T[u], tr[u])
    pf, pt, t_cpu = R.recompute(derivs, rows[u], feed[u], tr[u])
    assert np.all(R.is_root(derivs, rows[u], pf, tr[u], noise))
    assert np.all(np.abs(t_cpu - tpd[u]) <= 1e-9 + 2.0 * noise / tr[u].sum(axis=1)), np.abs(t_cpu - tpd[u]).max()
    assert np.all(t_cpu < -TPD_TOL)


def test_referee_agreement(oracle):
    (P, K, T, X, PI), out = _converged_feeds(1500)
    feeds, idx = [], []
    for dew in (False, True):
        ok, rho4, _ = out[dew]
        take = ok[:150]
        feeds.append(rho4[take, 0:2] if dew else rho4[take, 2:4])
        idx.append(take)
    # both solutions of the dew rows on which the kernel and the oracle's continuation solver land on different pressures
    ok, rho4, p_gpu = out[True]
    pC, rC, code, _ = oracle.mix_bubble_dew_continuation(P[ok], K[ok], T[ok], X[ok], True, prec=0)
    diff = (code == 0) & (np.abs(p_gpu[ok] - pC) > 1e-8 * np.abs(pC))
    feeds += [rho4[ok[diff], 0:2], rC[diff, 0:2]]
    idx += [ok[diff], ok[diff]]
    # liquids at perturbed compositions (same total density): inside and outside miscibility gaps
    ok, rho4, _ = out[False]
    take = ok[150:230]
    tot = rho4[take, 2:4].sum(axis=1)
    zz = np.clip(rho4[take, 2] / tot + np.where(np.arange(len(take)) % 2, 0.07, -0.07), 0.02, 0.98)
    feeds.append(np.stack([zz * tot, (1 - zz) * tot], axis=1))
    idx.append(take)
    feed, rows = np.concatenate(feeds), np.concatenate(idx)
    Pk, Kk, Tk = P[rows], K[rows], T[rows]
    s, tpd, tr = _stab(Pk, Kk, Tk, feed)
    d = R.mix_derivs(oracle, Pk, Kk, Tk)
    ref = R.tpd_minimum(d, R.mix_packing(Pk, Tk), feed)
    noise = R.mix_pressure_noise(oracle, Pk, Kk, Tk, feed)
    judged = noise <= 1e-6 * np.abs(ref["pf"])
    rt = ref["tpd"]
    print(f"{len(rows)} feeds ({diff.sum()} kernel / continuation pairs), {judged.sum()} judged; kernel status counts "
          f"{np.bincount(s, minlength=4)}; referee < -1e-5 on {(rt < -1e-5).sum()}")
    print(f"   agreement: both unstable {((rt < -1e-5) & (s != 0) & judged).sum()}, both stable {((rt >= -1e-5) & (s == 0) & judged).sum()}, "
          f"kernel unstable / referee within 1e-5 of 0 {((rt >= -1e-5) & (s != 0) & judged).sum()}")
    assert np.all(s[judged & (rt < -1e-5)] != 0)
    assert np.all(rt[judged & (s == 0)] >= -1e-5)
    _check_unstable(oracle, d, np.arange(len(rows)), Pk, Kk, Tk, feed, s, tpd, tr)


@pytest.mark.parametrize("dew", [False, True])
def test_check_stability_identity(dew):
    from feos_torch_amd import PcSaftMix, native
    from feos_torch_amd.synthetic import mix_batch

    n = 3000
    P, K, T, X, PI = mix_batch(n, seed=78)
    runs = []
    for check in (False, True):
        par = _d(P).requires_grad_(True)
        kij = _d(K).requires_grad_(True)
        temp = _d(T).requires_grad_(True)
        eos = PcSaftMix(par, kij)
        fn = eos.dew_point if dew else eos.bubble_point
        out = fn(temp, _d(X), _d(PI), check_stability=True) if check else fn(temp, _d(X), _d(PI))
        assert len(out) == (3 if check else 2)
        out[0].sum().backward()
        runs.append((out, par.grad, kij.grad, temp.grad, eos))
    (p0, n0), g0p, g0k, g0t, e0 = runs[0][0], runs[0][1], runs[0][2], runs[0][3], runs[0][4]
    (p1, n1, stable), g1p, g1k, g1t, e1 = runs[1][0], runs[1][1], runs[1][2], runs[1][3], runs[1][4]
    assert torch.equal(p0, p1) and torch.equal(n0, n1)
    assert torch.equal(g0p, g1p) and torch.equal(g0k, g1k) and torch.equal(g0t, g1t)
    assert torch.equal(e0._par, e1._par) and torch.equal(e0.kij, e1.kij)
    assert stable.dtype == torch.bool and stable.shape == p1.shape and not stable.requires_grad
    # = stability_analysis of the reduced model at the converged densities of the specified phase
    r = native.mix_bubble_dew(_d(P), _d(K), _d(T), _d(X), _d(PI), dew)
    ok = ~r["status"]
    feed = r["rho4"][ok][:, 0:2] if dew else r["rho4"][ok][:, 2:4]
    st2, tpd, trial = e1.stability_analysis(_d(T)[ok], feed)
    assert torch.equal(stable, st2)
    assert tpd.shape == (int(ok.sum()),) and trial.shape == (int(ok.sum()), 2) and not tpd.requires_grad
    print(f"{'dew' if dew else 'bubble'}: flagged {(~stable).float().mean().item():.4%} of {stable.numel()} converged rows")


def test_stability_analysis_has_no_graph_and_keeps_the_model():
    from feos_torch_amd import PcSaftMix

    par = _d(np.tile([[2.0, 3.5, 250.0, 0, 0, 0, 0, 0], [1.5, 3.2, 200.0, 0, 0, 0, 0, 0]], (4, 1, 1))).requires_grad_(True)
    eos = PcSaftMix(par)
    rho = _d(np.array([[1e-5, 1e-5], [0.0, 1e-3], [4e-3, 4e-3], [1e-4, 1e-7]])).requires_grad_(True)
    stable, tpd, trial = eos.stability_analysis(_d(np.full(4, 250.0)).requires_grad_(True), rho)
    assert not tpd.requires_grad and not trial.requires_grad and tpd.grad_fn is None
    assert eos._par.shape[0] == 4 and stable.shape == (4,) and not bool(stable[1])


def _gc_model(table, b, idx=None):
    from feos_torch_amd import GcPcSaftMix

    ident = [s for s, _ in table]
    seg = tuple(torch.tensor([v[k] for _, v in table], dtype=f64) for k in range(8))
    sl, bl = b["segment_lists"], b["bond_lists"]
    phi = np.asarray(b["phi"], dtype=np.float64)
    if idx is not None:
        sl, bl, phi = [sl[i] for i in idx], [bl[i] for i in idx], phi[idx]
    return GcPcSaftMix(ident, seg, sl, bl, b["kab_list"], torch.tensor(phi, dtype=f64))


def _gc_solve(eos, T, z, p0, dew):
    from feos_torch_amd import native

    table = eos._table()
    r = native.gc_bubble_dew(table, eos.S, eos.rows, native._prep(eos.phi, eos.device, (2,)), _d(T), _d(z), _d(p0), dew)
    return r


def test_gc_reference_cases_and_referee_agreement(oracle, table):
    from conftest import load_golden
    from feos_torch_amd.synthetic import gc_batch

    g = load_golden("gc.json")
    for key, dew in (("test_bubble", False), ("test_dew", True)):
        c = g[key]
        b = {"segment_lists": c["segment_lists"], "bond_lists": c["bond_lists"], "phi": c["phi"],
             "kab_list": [(s1, s2, k) for (s1, s2), k in zip(c["kab_pairs"], c["kab_vals"])]}
        eos = _gc_model(table, b)
        T = np.asarray(c["T"], dtype=np.float64)
        r = _gc_solve(eos, T, np.asarray(c["z"]), np.asarray(c["p_init"]), dew)
        assert not r["status"].any()
        rho4 = r["rho4"].cpu().numpy()
        feed = rho4[:, 0:2] if dew else rho4[:, 2:4]
        stable, tpd, _ = eos.stability_analysis(_d(T), _d(feed))
        enc = oracle.gc_encode(table, b["segment_lists"], b["bond_lists"], b["kab_list"])
        ref = R.tpd_minimum(R.gc_derivs(oracle, enc, np.asarray(b["phi"]), T), R.gc_packing(enc, T), feed)
        print(f"gc reference {key}: kernel stable {stable.tolist()} tpd {tpd.tolist()}; referee tpd {ref['tpd'].tolist()}")
        assert stable.tolist() == (ref["tpd"] >= -1e-5).tolist()
    # gc_batch feeds: 100 bubble + 100 dew
    n = 400
    b = gc_batch(n, table, seed=41)
    eos = _gc_model(table, b)
    enc = oracle.gc_encode(table, b["segment_lists"], b["bond_lists"], b["kab_list"])
    feeds, idx = [], []
    for dew in (False, True):
        r = _gc_solve(eos, b["T"], b["x"], b["p_init"], dew)
        ok = np.nonzero(~r["status"].cpu().numpy())[0][:100]
        rho4 = r["rho4"].cpu().numpy()
        feeds.append(rho4[ok, 0:2] if dew else rho4[ok, 2:4])
        idx.append(ok)
    feed, rows = np.concatenate(feeds), np.concatenate(idx)
    T = b["T"][rows]
    from feos_torch_amd import native

    table_d = eos._table()
    rows_d = eos.rows[_d(rows.astype(np.int64))].contiguous()
    phi_d = _d(np.asarray(b["phi"])[rows])
    res = native.gc_stability(table_d, eos.S, rows_d, phi_d, _d(T), _d(feed))
    s, tpd, tr = res["status"].cpu().numpy(), res["tpd"].cpu().numpy(), res["rho_trial"].cpu().numpy()
    e = dict(enc)
    e["counts"], e["bonds"] = enc["counts"][rows], enc["bonds"][rows]
    phi_r = np.asarray(b["phi"])[rows]
    d = R.gc_derivs(oracle, e, phi_r, T)
    ref = R.tpd_minimum(d, R.gc_packing(e, T), feed)
    noise = R.gc_pressure_noise(oracle, e, phi_r, T, feed)
    judged = noise <= 1e-6 * np.abs(ref["pf"])
    rt = ref["tpd"]
    print(f"gc: {len(rows)} feeds, {judged.sum()} judged; kernel status counts {np.bincount(s, minlength=4)}; referee < -1e-5 on "
          f"{(rt < -1e-5).sum()}")
    assert np.all(s[judged & (rt < -1e-5)] != 0)
    assert np.all(rt[judged & (s == 0)] >= -1e-5)
    u = np.nonzero(s == 1)[0]
    if len(u):
        pf, pt, t_cpu = R.recompute(d, u, feed[u], tr[u])
        nz = noise[u] + R.gc_pressure_noise(oracle, {**e, "counts": e["counts"][u], "bonds": e["bonds"][u]}, phi_r[u], T[u], tr[u])
        assert np.all(R.is_root(d, u, pf, tr[u], nz))
        assert np.all(np.abs(t_cpu - tpd[u]) <= 1e-9 + 2.0 * nz / tr[u].sum(axis=1))
        assert np.all(t_cpu < -TPD_TOL)
    # order = None and the class order: identical outputs
    order = native.gc_class_order(table_d, eos.S, rows_d)
    res2 = native.gc_stability(table_d, eos.S, rows_d, phi_d, _d(T), _d(feed), order=order)
    assert torch.equal(res["status"], res2["status"])
    assert torch.equal(res["tpd"].nan_to_num(0.0), res2["tpd"].nan_to_num(0.0))
    assert torch.equal(res["rho_trial"].nan_to_num(0.0), res2["rho_trial"].nan_to_num(0.0))


@pytest.mark.parametrize("dew", [False, True])
def test_gc_check_stability_identity(table, dew):
    from feos_torch_amd import GcPcSaftMix
    from feos_torch_amd.synthetic import gc_batch

    n = 2000
    b = gc_batch(n, table, seed=43)
    ident = [s for s, _ in table]
    runs = []
    for check in (False, True):
        seg = tuple(torch.tensor([v[k] for _, v in table], dtype=f64, requires_grad=True) for k in range(8))
        kab = torch.tensor([k[2] for k in b["kab_list"]], dtype=f64, requires_grad=True)
        kab_list = [(k[0], k[1], kv) for k, kv in zip(b["kab_list"], kab)]
        phi = torch.tensor(b["phi"], dtype=f64, requires_grad=True)
        temp = torch.tensor(b["T"], dtype=f64, requires_grad=True)
        eos = GcPcSaftMix(ident, seg, b["segment_lists"], b["bond_lists"], kab_list, phi)
        fn = eos.dew_point if dew else eos.bubble_point
        x, p0 = torch.tensor(b["x"], dtype=f64), torch.tensor(b["p_init"], dtype=f64)
        out = fn(temp, x, p0, check_stability=True) if check else fn(temp, x, p0)
        assert len(out) == (3 if check else 2)
        out[0].sum().backward()
        runs.append((out, [s.grad for s in seg], kab.grad, phi.grad, temp.grad, eos))
    a, bb = runs
    assert torch.equal(a[0][0], bb[0][0]) and torch.equal(a[0][1], bb[0][1])
    # the segment-parameter gradient is accumulated over the rows with fp64 atomics (pcs_gc_segment_gradient): its summation
    # order, and so its last bits, differ between any two calls, with or without the check
    for ga, gb in zip(a[1], bb[1]):
        assert (ga is None and gb is None) or torch.allclose(ga, gb, rtol=1e-12, atol=1e-12 * float(ga.abs().max()))
    assert torch.equal(a[2], bb[2]) and torch.equal(a[3], bb[3]) and torch.equal(a[4], bb[4])
    assert torch.equal(a[5].rows, bb[5].rows) and torch.equal(a[5].phi, bb[5].phi)
    stable = bb[0][2]
    assert stable.dtype == torch.bool and stable.shape == bb[0][0].shape and not stable.requires_grad
    eos = bb[5]
    r = _gc_solve(_gc_model(table, b), b["T"], b["x"], b["p_init"], dew)
    ok = ~r["status"]
    feed = r["rho4"][ok][:, 0:2] if dew else r["rho4"][ok][:, 2:4]
    st2, _, _ = eos.stability_analysis(_d(b["T"])[ok], feed)
    assert torch.equal(stable.to(st2.device), st2)
    print(f"gc {'dew' if dew else 'bubble'}: flagged {(~stable).float().mean().item():.4%} of {stable.numel()} converged rows")


def test_scale_1e6_dew_feeds():
    import ctypes  # noqa: F401

    from feos_torch_amd import _lib, native
    from feos_torch_amd.synthetic import mix_batch

    n = 1_000_000
    P, K, T, X, PI = mix_batch(n, seed=78)
    a = [_d(v) for v in (P, K, T, X, PI)]
    r = native.mix_bubble_dew(*a, True)
    ok = torch.nonzero(~r["status"]).view(-1)
    feed = r["rho4"][ok][:, 0:2].contiguous()
    Pk, Kk, Tk = a[0][ok].contiguous(), a[1][ok].contiguous(), a[2][ok].contiguous()
    native.mix_stability(Pk[:1000], Kk[:1000], Tk[:1000], feed[:1000])  # warm
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    res = native.mix_stability(Pk, Kk, Tk, feed)
    e1.record()
    torch.cuda.synchronize()
    cnt = torch.bincount(res["status"].long(), minlength=4).tolist()
    print(f"pcs_mix_stability on {len(ok)} converged dew feeds: {e0.elapsed_time(e1):.2f} ms; status counts {cnt}")
    assert cnt[3] == 0
    assert _lib.lib().pcs_last_error() == b""
