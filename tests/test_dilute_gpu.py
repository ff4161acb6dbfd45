"""GPU: the mixture kernels in the dilute limit, against the long-double references that tests/test_oracle_dilute.py pins
on the CPU.

Every other GPU mixture test draws its compositions from [0.1, 0.9], yet the kernels hold code that only a trace component
reaches: the trace step of the Newton iteration and its acceptance rules (csrc/mix_solver_sm.hpp), the Raoult start, the
trace-polar limit |phi2| < 1e-90 of the dipole term (csrc/mix_model.hpp, csrc/mix_adjoint.hpp and the gc twin) and the
stability search at a dilute feed.  Here the same seeded rows are solved on the grid DILUTE_Z (tests/tools/dilute_grid.py)
and the state functions are evaluated at trace partial densities.  Each tolerance is that of the existing test of the same
quantity (named in the docstrings); the measured maximum error is printed next to it."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import stability_referee as R  # noqa: E402
from dilute_grid import DILUTE_Z, grid, henry_error, trace_index  # noqa: E402

pytestmark = pytest.mark.gpu
f64 = torch.float64
N_MIX = 600
N_GC = 300
# the kernels also run at 1 - 2^-46: the mirror of the pure-component limit at 2^-46 (no oracle column)
Z_GPU = DILUTE_Z + (1.0 - 2.0**-46,)
# rho_trace / rho: both sides of the trace-polar switch |phi2| < PHI2_TRACE = 1e-60 (csrc/pcsaft_consts.hpp; phi2 ~ rho_polar^2,
# so the switch sits near rho_polar / rho ~ 1e-29), among them 1e-44, where the former threshold 1e-90 let the backward pass
# overflow
TRACE_RATIOS = (0.0, 1e-300, 1e-60, 1e-46, 1e-44, 1e-29, 1e-20, 1e-8)


def _d(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _np(x):
    return x.detach().cpu().numpy()


@pytest.fixture(scope="module")
def amd():
    assert torch.cuda.is_available()
    import feos_torch_amd

    return feos_torch_amd


@pytest.fixture(scope="module")
def table():
    from feos_torch_amd.synthetic import load_segment_table

    return load_segment_table(os.path.join(ROOT, "tests", "data", "sauer2014_hetero.json"))


def _single_pass(dew, a):
    """pcs_mix_bubble_dew with workspace = NULL: one row per lane, no work queue, no pre-pass."""
    from feos_torch_amd import _lib

    n = a[2].shape[0]
    p = torch.empty(n, dtype=f64, device="cuda")
    rho4 = torch.empty((n, 4), dtype=f64, device="cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    rc = _lib.lib().pcs_mix_bubble_dew(int(dew), *[_lib.ptr(v) for v in a], n, _lib.ptr(p), _lib.ptr(rho4), _lib.ptr(st), None,
                                       None, _lib.current_stream_ptr(p.device))
    assert rc == 0
    torch.cuda.synchronize()
    return {"p": p, "rho4": rho4, "status": st.bool()}


@pytest.fixture(scope="module")
def mix():
    from feos_torch_amd.synthetic import mix_batch

    P, K, T, _, PI = mix_batch(N_MIX, seed=91)
    return P, K, T, PI


@pytest.fixture(scope="module")
def mix_solved(oracle, mix):
    """{dew: dict(p, rho4, st: the work-queue kernel [N_MIX, len(Z_GPU)]; single: the workspace = NULL run of the same rows;
    op, orho4, ost: the long-double oracle [N_MIX, len(DILUTE_Z)])}"""
    from feos_torch_amd import native

    P, K, T, PI = mix
    i, z = grid(N_MIX, Z_GPU)
    io, zo = grid(N_MIX, DILUTE_Z)
    G, Go = len(Z_GPU), len(DILUTE_Z)
    out = {}
    for dew in (False, True):
        a = [_d(v) for v in (P[i], K[i], T[i], z, PI[i])]
        r = native.mix_bubble_dew(*a, dew, want_iters=True)
        single = _single_pass(dew, a)
        p, rho4, st = oracle.mix_bubble_dew(P[io], K[io], T[io], zo, PI[io], dew, prec=1)
        out[dew] = dict(p=_np(r["p"]).reshape(N_MIX, G), rho4=_np(r["rho4"]).reshape(N_MIX, G, 4), st=_np(r["status"]).reshape(N_MIX, G),
                        queue=r, single=single, op=p.reshape(N_MIX, Go), orho4=rho4.reshape(N_MIX, Go, 4), ost=st.reshape(N_MIX, Go))
    return out


@pytest.mark.parametrize("dew", [False, True])
def test_bubble_dew_vs_oracle(mix_solved, dew):
    """tests/test_mix_gpu.py::test_random_batch_vs_oracle on the dilute grid: failure masks differ on at most 1 % of the rows,
    p to 1e-9 relative; the trace component's partial density in the incipient phase to 1e-7 of ITSELF (an absolute
    comparison would pass trivially).  The workspace = NULL schedule solves the same rows (tolerances of
    test_single_pass_schedule_without_workspace)."""
    m = mix_solved[dew]
    Go = len(DILUTE_Z)
    st, ost = m["st"][:, :Go], m["ost"]
    per_z = (st != ost).sum(axis=0)
    both = ~st & ~ost
    errp = np.abs(m["p"][:, :Go][both] / m["op"][both] - 1)
    inc = slice(2, 4) if dew else slice(0, 2)
    tr = trace_index(np.broadcast_to(np.asarray(DILUTE_Z), st.shape)[both])
    k = np.arange(len(tr))
    errt = np.abs(m["rho4"][:, :Go][both][:, inc][k, tr] / m["orho4"][both][:, inc][k, tr] - 1)
    print(f"{'dew' if dew else 'bubble'}: masks differ on {per_z.tolist()} rows per z of {N_MIX} (tol 1 %); failed "
          f"{st.sum(axis=0).tolist()}; max |p / p_oracle - 1| {errp.max():.2e} (tol 1e-9); trace partial density of the incipient "
          f"phase {errt.max():.2e} relative (tol 1e-7)")
    assert (st != ost).mean() < 0.01
    assert errp.max() < 1e-9
    assert errt.max() < 1e-7
    q, s = m["queue"], m["single"]
    ok = ~q["status"]
    assert torch.equal(s["status"], q["status"])
    assert torch.allclose(s["p"][ok], q["p"][ok], rtol=1e-11, atol=0.0) and torch.allclose(s["rho4"][ok], q["rho4"][ok], rtol=1e-10, atol=0.0)


@pytest.mark.parametrize("dew,cap", [(False, 6), (True, 20)])
def test_trace_newton_steps_do_not_march(mix_solved, dew, cap):
    """The Newton iteration takes the step of a trace component of the incipient phase unscaled (its chemical potential is
    linear in ln rho_i, csrc/mix_solver_sm.hpp NEWTON_TRACE), so the dilute rows converge in a few iterations: measured at
    most 4 (bubble) and 14 (dew) on this grid.  With every step scaled to a factor e the bubble rows march (up to 17)."""
    m = mix_solved[dew]
    ok = ~m["queue"]["status"]
    it = _np(m["queue"]["iters"][ok])
    print(f"{'dew' if dew else 'bubble'}: Newton iterations on {ok.sum().item()} dilute rows: max {it.max()}, mean {it.mean():.2f} "
          f"(cap {cap})")
    assert it.max() <= cap


@pytest.mark.parametrize("dew", [False, True])
def test_pure_component_limit_across_kernels(amd, mix, mix_solved, dew):
    """At z = 2^-46 the mixture kernel's p is PcSaftPure.vapor_pressure of component 2 plus the Henry term s z (s = chord of
    the mixture kernel's p at 2^-30 and 2^-20); the mirror at 1 - 2^-46 against component 1 (chord at 1 - 2^-40 and
    1 - 2^-20).  1e-9 relative, that of p (tests/test_oracle_dilute.py::test_mix_pure_component_limit on the CPU)."""
    P, K, T, PI = mix
    m = mix_solved[dew]
    col = {z: j for j, z in enumerate(Z_GPU)}
    for comp, zs, ds in ((1, (2.0**-46, 2.0**-30, 2.0**-20), (2.0**-46, 2.0**-30, 2.0**-20)),
                         (0, (1 - 2.0**-46, 1 - 2.0**-40, 1 - 2.0**-20), (2.0**-46, 2.0**-40, 2.0**-20))):
        nans, vp = amd.PcSaftPure(_d(P[:, comp])).vapor_pressure(_d(T))
        nans = _np(nans)
        psat = np.ones(N_MIX)
        psat[~nans] = _np(vp)
        cols = [col[z] for z in zs]
        err, judged = henry_error(*(m["p"][:, c] for c in cols), *ds, psat)
        ok = ~nans & ~m["st"][:, cols].any(axis=1)
        sel = ok & judged
        print(f"{'dew' if dew else 'bubble'}, component {comp + 1} remains: {sel.sum()} rows judged ({(ok & ~judged).sum()} not "
              f"Henry-linear), max |p - p_sat - s d| / p_sat {err[sel].max():.2e} (tol 1e-9)")
        assert sel.sum() >= 0.6 * N_MIX
        assert err[sel].max() < 1e-9


@pytest.mark.parametrize("dew", [False, True])
def test_jacobian_and_autograd(amd, oracle, mix, mix_solved, dew):
    """tests/test_mix_gpu.py::test_jacobian_vs_oracle on the dilute grid (pcs_mix_jacobian at the kernel's rho4 against the
    exact gradient, 1e-8 of the row scale); autograd through bubble_point / dew_point is finite on every converged row."""
    from feos_torch_amd import native

    P, K, T, PI = mix
    m = mix_solved[dew]
    i, z = grid(N_MIX, Z_GPU)
    ok = ~m["st"].ravel()
    rho4 = m["rho4"].reshape(-1, 4)[ok]
    Pk, Kk, Tk = P[i][ok], K[i][ok], T[i][ok]
    J = _np(native.mix_jacobian(_d(Pk), _d(Kk), _d(Tk), _d(rho4), dew))
    _, want = oracle.mix_bubble_dew_grad(Pk, Kk, Tk, rho4, dew, exact=True)
    err = np.abs(J - want) / np.abs(want).max(axis=1, keepdims=True)
    sites = [6, 7, 14, 15]  # d/d(na, nb) of both components
    rest = [k for k in range(19) if k not in sites]
    print(f"{'dew' if dew else 'bubble'} Jacobian vs exact on {ok.sum()} dilute rows: max {err[:, rest].max():.2e} (tol 1e-8); "
          f"d/d(na, nb) {err[:, sites].max():.2e} (tol 1e-7)")
    assert err[:, rest].max() < 1e-8
    # d/d(na, nb) of a self-associating component next to a trace of the other: up to 4.7e-8 of the row scale (one-sided
    # association, z = 2^-46), where the fp64 restatement of the same formulas is within 1e-14 -- a precision gap of the
    # adjoint kernel that this bound records rather than hides
    assert err[:, sites].max() < 1e-7
    par, kij, temp = _d(P[i]).requires_grad_(True), _d(K[i]).requires_grad_(True), _d(T[i]).requires_grad_(True)
    eos = amd.PcSaftMix(par, kij)
    p, nans = (eos.dew_point if dew else eos.bubble_point)(temp, _d(z), _d(PI[i]))
    assert np.array_equal(_np(nans), ~ok)
    p.sum().backward()
    conv = ~nans
    assert bool(torch.isfinite(par.grad[conv]).all() and torch.isfinite(kij.grad[conv]).all() and torch.isfinite(temp.grad[conv]).all())


@pytest.mark.parametrize("dew", [False, True])
def test_edge_compositions(amd, oracle, mix, dew):
    """Contract 0 < z < 1 (include/pcsaft_hip.h): z = 0 and z = 1 come back failed, as in the oracle.  Below the grid, at
    z = 1e-300 and 5e-324 (subnormal), a row either fails or equals its result at z = 1e-100 to 1e-12 -- and at 1e-100 the
    Henry term is below rounding on every row, so that result is the vapour pressure of component 2 (1e-9, that of p) and the
    oracle's (1e-9).  Both schedules."""
    from feos_torch_amd import native

    P, K, T, PI = mix
    zs = (0.0, 1.0, 1e-100, 1e-300, 5e-324)
    i, z = grid(N_MIX, zs)
    a = [_d(v) for v in (P[i], K[i], T[i], z, PI[i])]
    want, _, wst = oracle.mix_bubble_dew(P, K, T, np.full(N_MIX, 1e-100), PI, dew, prec=1)
    nans, vp = amd.PcSaftPure(_d(P[:, 1])).vapor_pressure(_d(T))
    nans = _np(nans)
    psat = np.ones(N_MIX)
    psat[~nans] = _np(vp)
    for name, r in (("queue", native.mix_bubble_dew(*a, dew)), ("single pass", _single_pass(dew, a))):
        st = _np(r["status"]).reshape(N_MIX, len(zs))
        p = _np(r["p"]).reshape(N_MIX, len(zs))
        assert st[:, 0].all() and st[:, 1].all(), name
        ok = ~st[:, 2]
        both = ok & ~wst
        e_orc = np.abs(p[both, 2] / want[both] - 1)
        e_sat = np.abs(p[ok & ~nans, 2] / psat[ok & ~nans] - 1)
        assert (ok != ~wst).mean() < 0.01 and ok.mean() > 0.97
        worst = 0.0
        for c in (3, 4):
            okc = ~st[:, c] & ok
            e = np.abs(p[okc, c] / p[okc, 2] - 1)
            worst = max(worst, float(np.max(e, initial=0.0)))
            assert np.all(e < 1e-12), (name, zs[c], e.max())
        print(f"{'dew' if dew else 'bubble'} {name}: z = 1e-100 vs oracle {e_orc.max():.2e}, vs p_sat {e_sat.max():.2e} (tol 1e-9); "
              f"z = 1e-300 / 5e-324 converged on {(~st[:, 3]).sum()} / {(~st[:, 4]).sum()} rows, max difference to z = 1e-100 "
              f"{worst:.2e} (tol 1e-12)")
        assert e_orc.max() < 1e-9 and e_sat.max() < 1e-9


def test_bubble_rows_at_1e300_converge(amd):
    """Bubble rows at z = 1e-300 (liquid trace density ~1e-302, still normal; the incipient vapour's is often subnormal, so its
    Newton steps stop shrinking on the rounding floor): the stagnation acceptance (NEWTON_FLOOR, csrc/mix_solver_sm.hpp)
    carries them.  Measured on these 6000 rows: 64 fail at 1e-300 (none at 1e-100); without that acceptance 86 fail.  Every
    converged row equals its z = 1e-100 result to 1e-12 (test_edge_compositions)."""
    from feos_torch_amd import native
    from feos_torch_amd.synthetic import mix_batch

    n = 6000
    P, K, T, _, PI = mix_batch(n, seed=91)
    i, z = grid(n, (1e-100, 1e-300))
    r = native.mix_bubble_dew(*(_d(v) for v in (P[i], K[i], T[i], z, PI[i])), False)
    st = _np(r["status"]).reshape(n, 2)
    p = _np(r["p"]).reshape(n, 2)
    both = ~st[:, 0] & ~st[:, 1]
    e = np.abs(p[both, 1] / p[both, 0] - 1)
    print(f"bubble: failed at z = 1e-100 / 1e-300: {st[:, 0].sum()} / {st[:, 1].sum()} of {n} (cap 0 / 72); max difference "
          f"{e.max():.2e} (tol 1e-12)")
    assert st[:, 0].sum() == 0 and st[:, 1].sum() <= 72
    assert e.max() < 1e-12


# ---------------------------------------------------------------------------------------------------------------------------
# gc bubble / dew
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gc_grid(oracle, table):
    from feos_torch_amd.synthetic import gc_batch

    b = gc_batch(N_GC, table, seed=93)
    i, z = grid(N_GC, DILUTE_Z)
    segs, bonds = [b["segment_lists"][k] for k in i], [b["bond_lists"][k] for k in i]
    enc = oracle.gc_encode(table, segs, bonds, b["kab_list"])
    g = dict(kab_list=b["kab_list"], segs=segs, bonds=bonds, enc=enc, phi=b["phi"][i], T=b["T"][i], z=z, PI=b["p_init"][i])
    g["ref"] = {dew: oracle.gc_bubble_dew(enc, g["phi"], g["T"], z, g["PI"], dew, prec=1) for dew in (False, True)}
    return g


def _gc_model(amd, table, segs, bonds, kab_list, phi, seg_grad=False):
    ident = [s for s, _ in table]
    cols = tuple(torch.tensor([v[k] for _, v in table], dtype=f64, requires_grad=seg_grad) for k in range(8))
    return amd.GcPcSaftMix(ident, cols, segs, bonds, kab_list, phi), cols


@pytest.mark.parametrize("dew", [False, True])
def test_gc_bubble_dew_vs_oracle(amd, oracle, table, gc_grid, dew):
    """tests/test_gc_gpu.py::test_random_rows_vs_oracle on the dilute grid: masks, p to 1e-9, d/dk_ab summed over the rows,
    d/dphi and d/dT to 1e-7 against the long-double gradient; the trace partial density of the incipient phase to 1e-7 of
    itself."""
    from feos_torch_amd import native

    g = gc_grid
    n = len(g["z"])
    kab = torch.tensor([k[2] for k in g["kab_list"]], dtype=f64, requires_grad=True)
    kab_list = [(k[0], k[1], kv) for k, kv in zip(g["kab_list"], kab)]
    phi = torch.tensor(g["phi"], dtype=f64, requires_grad=True)
    T = torch.tensor(g["T"], dtype=f64, requires_grad=True)
    eos, _ = _gc_model(amd, table, g["segs"], g["bonds"], kab_list, phi)
    raw = native.gc_bubble_dew(eos._table(), eos.S, eos.rows, _d(g["phi"]), _d(g["T"]), _d(g["z"]), _d(g["PI"]), dew)
    p, nans = (eos.dew_point if dew else eos.bubble_point)(T, torch.tensor(g["z"], dtype=f64), torch.tensor(g["PI"], dtype=f64))
    want, rho4, st = g["ref"][dew]
    nn = _np(nans)
    assert np.array_equal(nn, _np(raw["status"]))
    got = np.zeros(n)
    got[~nn] = _np(p)
    both = ~nn & ~st
    errp = np.abs(got[both] / want[both] - 1)
    inc = slice(2, 4) if dew else slice(0, 2)
    tr = trace_index(g["z"][both])
    k = np.arange(len(tr))
    errt = np.abs(_np(raw["rho4"])[both][:, inc][k, tr] / rho4[both][:, inc][k, tr] - 1)
    p.sum().backward()
    _, grad = oracle.gc_bubble_dew_grad(g["enc"], g["phi"], g["T"], rho4, dew, "CH3", "CH2", exact=True)
    ik = [kk[:2] for kk in g["kab_list"]].index(("CH3", "CH2"))
    wk = grad[both, 0].sum()
    ek = abs(kab.grad[ik].item() - wk - grad[~nn & st, 0].sum())
    gp = _np(phi.grad)[both]
    rel_p = (np.abs(gp - grad[both, 1:3]) / np.abs(grad[both, 1:3]).max(axis=1, keepdims=True)).max(axis=1)
    rel_t = np.abs(_np(T.grad)[both] / grad[both, 3] - 1)
    print(f"gc {'dew' if dew else 'bubble'}: masks differ on {(nn != st).sum()} of {n} rows, failed {nn.sum()}; p {errp.max():.2e} "
          f"(tol 1e-9); trace partial density {errt.max():.2e} (tol 1e-7); dp/dk_ab sum {ek / abs(wk):.2e} relative; dp/dphi "
          f"{rel_p.max():.2e}, dp/dT {rel_t.max():.2e} (tol 1e-7)")
    assert (nn != st).mean() < 0.01 and nn.mean() < 0.03
    assert errp.max() < 1e-9 and errt.max() < 1e-7
    assert ek < 1e-6 * abs(wk) + 1e-3 * (nn != st).sum()
    assert rel_p.max() < 1e-7 and rel_t.max() < 1e-7


@pytest.mark.parametrize("dew", [False, True])
def test_gc_edge_compositions(amd, table, gc_grid, dew):
    """The contract 0 < z < 1 for gc rows (the same solver as the binary rows, include/pcsaft_hip.h): z = 0 and 1 fail; at
    z = 1e-300 a row either fails or equals its result at z = 1e-100 to 1e-12."""
    from feos_torch_amd import native

    g = gc_grid
    G = len(DILUTE_Z)
    base = np.arange(0, len(g["z"]), G)  # one entry per gc row
    zs = (0.0, 1.0, 1e-100, 1e-300)
    k = np.repeat(base, len(zs))
    z = np.tile(np.asarray(zs), len(base))
    eos, _ = _gc_model(amd, table, [g["segs"][r] for r in k], [g["bonds"][r] for r in k], g["kab_list"], torch.tensor(g["phi"][k], dtype=f64))
    r = native.gc_bubble_dew(eos._table(), eos.S, eos.rows, _d(g["phi"][k]), _d(g["T"][k]), _d(z), _d(g["PI"][k]), dew)
    st = _np(r["status"]).reshape(len(base), len(zs))
    p = _np(r["p"]).reshape(len(base), len(zs))
    assert st[:, 0].all() and st[:, 1].all()
    assert (~st[:, 2]).mean() > 0.97
    both = ~st[:, 2] & ~st[:, 3]
    e = np.abs(p[both, 3] / p[both, 2] - 1)
    print(f"gc {'dew' if dew else 'bubble'}: z = 1e-100 converged on {(~st[:, 2]).sum()} of {len(base)}, z = 1e-300 on "
          f"{(~st[:, 3]).sum()}; max difference {np.max(e, initial=0.0):.2e} (tol 1e-12)")
    assert np.all(e < 1e-12)


def test_gc_segment_gradient_at_dilute_rows(amd, oracle, table, gc_grid):
    """pcs_gc_segment_gradient (autograd to the segment table) on a dozen dilute rows against central differences of the
    oracle's forward evaluation (tests/test_gc_seggrad_gpu.py::test_random_batch_vs_oracle_finite_differences: 5e-6 of the
    column scale)."""
    g = gc_grid
    G = len(DILUTE_Z)
    rng = np.random.default_rng(5)
    worst = 0.0
    for dew in (False, True):
        st = g["ref"][dew][2]
        # six rows, each at its most dilute composition on one side or the other
        cand = [r * G + (0 if r % 2 else G - 1) for r in range(N_GC)]
        pick = np.array([c for c in cand if not st[c]][:6])
        phi = g["phi"][pick]
        segs, bonds = [g["segs"][c] for c in pick], [g["bonds"][c] for c in pick]
        eos, cols = _gc_model(amd, table, segs, bonds, g["kab_list"], torch.tensor(phi, dtype=f64), seg_grad=True)
        p, nans = (eos.dew_point if dew else eos.bubble_point)(torch.tensor(g["T"][pick], dtype=f64),
                                                               torch.tensor(g["z"][pick], dtype=f64), torch.tensor(g["PI"][pick], dtype=f64))
        assert not bool(nans.any())
        w = rng.uniform(0.5, 1.5, len(pick))
        (p * torch.tensor(w, dtype=f64)).sum().backward()
        grad = np.stack([c.grad.numpy() for c in cols], axis=1)  # [S, 8]
        assert np.all(np.isfinite(grad))
        enc = oracle.gc_encode(table, segs, bonds, g["kab_list"])
        fd = oracle.gc_segment_grad_fd(enc, phi, g["T"][pick], g["ref"][dew][1][pick], dew, weights=w)
        for k in range(8):
            scale = np.max(np.abs(fd[:, k]))
            mask = fd[:, k] != 0.0
            if scale > 0:
                err = np.max(np.abs(grad[:, k][mask] - fd[:, k][mask])) / scale
                worst = max(worst, err)
                assert err < 5e-6, (dew, k, err)
    print(f"gc segment gradient on 12 dilute rows vs finite differences: max {worst:.2e} of the column scale (tol 5e-6)")


# ---------------------------------------------------------------------------------------------------------------------------
# state functions at trace partial density
# ---------------------------------------------------------------------------------------------------------------------------
def _trace_states(tot, ratios=TRACE_RATIOS):
    """rows [S], rho [S,2], ratio [S], trace component [S]: every (row, phase, trace component, ratio) combination; tot [2,2,n]
    = total densities of converged (vapour, liquid) phases with a trace of (component 1, component 2)"""
    rows, rho, q, c = [], [], [], []
    n = tot.shape[2]
    for ph in (0, 1):
        for tc in (0, 1):
            for r in ratios:
                x = np.zeros((n, 2))
                x[:, tc] = r * tot[ph, tc]
                x[:, 1 - tc] = (1.0 - r) * tot[ph, tc]
                rows.append(np.arange(n))
                rho.append(x)
                q.append(np.full(n, r))
                c.append(np.full(n, tc))
    return np.concatenate(rows), np.concatenate(rho), np.concatenate(q), np.concatenate(c)




def _dilution(mu, v, n):
    """States laid out by _trace_states: per ratio, the largest |mu_c(ratio) - mu_c(0)| / max(1, |mu_c(0)|) and
    |v_c(ratio) / v_c(0) - 1| of the trace component c over rows, phases and c."""
    M = mu.reshape(2, 2, len(TRACE_RATIOS), n, 2)
    V = v.reshape(2, 2, len(TRACE_RATIOS), n, 2)
    dm = np.stack([np.abs(M[ph, c, :, :, c] - M[ph, c, 0:1, :, c]) / np.maximum(1.0, np.abs(M[ph, c, 0:1, :, c]))
                   for ph in (0, 1) for c in (0, 1)])
    dv = np.stack([np.abs(V[ph, c, :, :, c] / V[ph, c, 0:1, :, c] - 1.0) for ph in (0, 1) for c in (0, 1)])
    return dm.max(axis=(0, 2)), dv.max(axis=(0, 2))


def _errors(a, p, mu, v, A, Pp, MU, V, rho):
    """per state: a, p, mu relative to their scale, v relative (the measures of tests/test_mix_gpu.py::test_derivatives_random_rows)"""
    return (np.abs(a - A) / np.maximum(np.abs(A), 1e-6), np.abs(p - Pp) / np.maximum(np.abs(Pp), rho.sum(axis=1)),
            (np.abs(mu - MU) / np.maximum(1.0, np.abs(MU))).max(axis=1), np.abs(v / V - 1.0).max(axis=1))


def _report(name, errs, q, tols):
    worst = [max(e.max() for e in errs[k:k + 1]) for k in range(4)]
    per = {f"{r:g}": float(max(e[q == r].max() for e in errs)) for r in np.unique(q)}
    tol = [float(np.max(t)) for t in tols]
    print(f"{name}: a {worst[0]:.2e} p {worst[1]:.2e} mu {worst[2]:.2e} v {worst[3]:.2e} (tol up to {tol}); worst per ratio {per}")
    for e, t in zip(errs, tols):
        assert np.all(e < t)


@pytest.fixture(scope="module")
def totals(mix_solved):
    """(rows, tot [2,2,n]): total densities of the (vapour, liquid) of the oracle's converged bubble rows at z = 2^-20 (trace of
    component 1) and 1 - 2^-20 (trace of component 2): densities of real phases of these rows, not a fixed number (at a fixed
    0.01 A^-3 some rows are non-finite even in the oracle, and a liquid density of one component can lie beyond close packing
    for the other)"""
    m = mix_solved[False]
    j0, j1 = DILUTE_Z.index(2.0**-20), DILUTE_Z.index(1.0 - 2.0**-20)
    rows = np.nonzero(~m["ost"][:, j0] & ~m["ost"][:, j1])[0][:240]
    r0, r1 = m["orho4"][rows, j0], m["orho4"][rows, j1]
    tot = np.array([[r0[:, 0:2].sum(axis=1), r1[:, 0:2].sum(axis=1)], [r0[:, 2:4].sum(axis=1), r1[:, 2:4].sum(axis=1)]])
    return rows, tot


def _fd_check(g, X, L, skip, rho_cols, tot):
    """central differences (relative step 1e-6) of L(X) [n] per column of X [n,k] against the analytic g [n,k]; entries that are
    0 are not perturbed, except density columns, where a trace density (below 1e-6 of the total) takes forward steps of
    1e-6 and 5e-7 of the total, extrapolated (Richardson).  -> max of |g - fd| / max(|fd|, 1e-6 row scale) (the measure of
    tests/test_mixn_gpu.py::test_vjp_vs_finite_differences_of_the_oracle)"""
    n, k = X.shape
    fd = g.copy()
    for j in range(k):
        if j in skip:
            continue
        x = X[:, j]
        if j in rho_cols:
            fwd = x < 1e-6 * tot
            h = np.where(fwd, 1e-6 * tot, 1e-6 * x)
        else:
            fwd = np.zeros(n, dtype=bool)
            h = 1e-6 * np.abs(x)
        mask = h > 0
        Xp, Xm, Xh = X.copy(), X.copy(), X.copy()
        Xp[:, j] += h
        Xm[:, j] = np.where(fwd, x, x - h)
        Xh[:, j] += 0.5 * h
        d = (L(Xp) - L(Xm)) / np.where(fwd, h, 2 * h)
        if fwd.any():  # forward steps: Richardson extrapolation of the steps h and h/2 (first-order error removed)
            d = np.where(fwd, 2.0 * (L(Xh) - L(Xm)) / (0.5 * h) - d, d)
        fd[:, j] = np.where(mask, d, g[:, j])
    cols = [j for j in range(k) if j not in skip]
    scale = np.abs(fd[:, cols]).max(axis=1, keepdims=True) + 1e-300
    err = np.abs(g[:, cols] - fd[:, cols]) / np.maximum(np.abs(fd[:, cols]), 1e-6 * scale)
    bad = ~np.isfinite(g).all(axis=1)
    assert not bad.any(), f"non-finite gradient on {bad.sum()} of {n} states"
    w, wc = np.unravel_index(np.argmax(err), err.shape)
    print(f"   worst finite-difference entry: state {w}, column {cols[wc]}: analytic {g[w, cols[wc]]:.10e}, fd {fd[w, cols[wc]]:.10e}, "
          f"row scale {scale[w, 0]:.3e}, x {X[w, cols[wc]]:.3e}")
    return float(err.max())


def test_mix_state_functions_at_trace_density(amd, oracle, mix, totals):
    """PcSaftMix.derivatives at rho_trace / rho in TRACE_RATIOS (both sides of the trace-polar switch; classes of mix_batch:
    polar, self-, cross- and induced association) against the exact values, tolerances of
    tests/test_mix_gpu.py::test_derivatives_random_rows.  Infinite dilution: mu and v of the trace component at 1e-300 equal
    those at 0 to 1e-14, and move by less than 1e-13 up to 1e-29, across the trace-polar switch."""
    P, K, T, _ = mix
    rows0, tot = totals
    n = len(rows0)
    idx, rho, q, _ = _trace_states(tot)
    rows = rows0[idx]
    a, p, mu, v = (_np(x) for x in amd.PcSaftMix(_d(P[rows]), _d(K[rows])).derivatives(_d(T[rows]), _d(rho)))
    assert all(np.all(np.isfinite(x)) for x in (a, p, mu, v))
    A, Pp, MU, V = oracle.mix_derivatives_exact(P[rows], K[rows], T[rows], rho)
    # dense, nearly pure associating liquids: the tolerance grows by 10 x the measured error of the same formulas in fp64 (the
    # oracle's double-precision restatement), as tests/test_oracle_mix.py::test_bubble_dew_random_rows does.  v: 1e-8, not the
    # 1e-10 of the random rows -- measured up to 4.9e-9 on these liquids (1.2e-9 at rho_trace / rho = 1e-8), an accuracy gap of
    # the partial molar volumes that this bound records
    noise = _errors(*oracle.mix_derivatives(P[rows], K[rows], T[rows], rho, robust=True), A, Pp, MU, V, rho)
    _report("binary", _errors(a, p, mu, v, A, Pp, MU, V, rho), q,
            tuple(t + 10.0 * e for t, e in zip((1e-13, 1e-12, 1e-13, 1e-8), noise)))
    dm, dv = _dilution(mu, v, n)
    print(f"   infinite dilution: |d mu_trace| {dict(zip(TRACE_RATIOS[1:], dm[1:].round(17)))}, |d v_trace| {dict(zip(TRACE_RATIOS[1:], dv[1:].round(17)))}")
    assert dm[1] < 1e-14 and dv[1] < 1e-14
    assert np.all(dm[1:6] < 1e-13) and np.all(dv[1:6] < 1e-13)  # across the switch (1e-44 | 1e-29)


def test_mix_backward_at_trace_density(amd, oracle, mix, totals):
    """pcs_mix_derivatives_vjp (through autograd) at the trace densities (zero included) of test_mix_state_functions_at_trace_density:
    finite, and against long-double central differences (tolerance of
    tests/test_mixn_gpu.py::test_vjp_vs_finite_differences_of_the_oracle)."""
    P, K, T, _ = mix
    rows0, tot = totals
    idx, rho, q, _ = _trace_states(tot)
    rows = rows0[idx]
    sub = np.nonzero(np.isin(idx, np.arange(8)))[0]
    Ps, Ks, Ts, rs = P[rows[sub]], K[rows[sub]], T[rows[sub]], rho[sub]
    m = len(sub)
    rng = np.random.default_rng(3)
    ga, gp, gmu, gv = rng.normal(size=m), rng.normal(size=m), rng.normal(size=(m, 2)), rng.normal(size=(m, 2)) * 1e-3
    par, kij, temp, den = (_d(x).requires_grad_(True) for x in (Ps, Ks, Ts, rs))
    a_, p_, mu_, v_ = amd.PcSaftMix(par, kij).derivatives(temp, den)
    ((a_ * _d(ga)).sum() + (p_ * _d(gp)).sum() + (mu_ * _d(gmu)).sum() + (v_ * _d(gv)).sum()).backward()
    g = np.concatenate([_np(par.grad).reshape(m, 16), _np(kij.grad), _np(temp.grad)[:, None], _np(den.grad)], axis=1)
    X = np.concatenate([Ps.reshape(m, 16), Ks, Ts[:, None], rs], axis=1)

    def L(X_):
        A_, P_, MU_, V_ = oracle.mix_derivatives_exact(X_[:, :16].reshape(m, 2, 8), X_[:, 16:18], X_[:, 18], X_[:, 19:21])
        return ga * A_ + gp * P_ + (gmu * MU_).sum(axis=1) + (gv * V_).sum(axis=1)

    err = _fd_check(g, X, L, skip={6, 7, 14, 15}, rho_cols={19, 20}, tot=rs.sum(axis=1))
    print(f"   backward vs long-double central differences on {m} states: {err:.2e} (tol 2e-4)")
    assert err < 2e-4


def _mixn_states(P2, T2, tv, tl, nc, rng):
    """nc components: the two of a binary row (rows of mix_batch classes 0-2: at most one associating component) and nc - 2
    non-associating draws; the totals scaled to the packing fraction of the binary phase; component 0 (and for odd rows also
    component nc - 1) at rho_trace / rho = ratio.  -> params [S,nc,8], T [S], rho [S,nc], ratio [S], trace mask [S,nc]"""
    n = len(T2)
    P = np.zeros((n, nc, 8))
    P[:, :2] = P2
    P[:, 2:, 0] = rng.uniform(1.0, 3.0, (n, nc - 2))
    P[:, 2:, 1] = rng.uniform(2.8, 4.2, (n, nc - 2))
    P[:, 2:, 2] = rng.uniform(150.0, 350.0, (n, nc - 2))
    P[:, 2:, 3] = np.where(rng.random((n, nc - 2)) < 0.4, rng.uniform(0.5, 3.0, (n, nc - 2)), 0.0)
    d3 = P[:, :, 0] * (P[:, :, 1] * (1 - 0.12 * np.exp(-3 * P[:, :, 2] / T2[:, None]))) ** 3
    trace = np.zeros((n, nc), dtype=bool)
    trace[:, 0] = True
    trace[1::2, nc - 1] = True
    x = rng.dirichlet(np.ones(nc), n) * ~trace
    x /= x.sum(axis=1, keepdims=True)
    out = []
    for tot in (tv, tl):
        eta = tot * d3[:, 1]  # the binary phase is (almost) pure component 2
        for r in TRACE_RATIOS:
            xr = np.where(trace, r, x * (1.0 - r * trace.sum(axis=1, keepdims=True)))
            out.append((P, T2, xr * (eta / (xr * d3).sum(axis=1))[:, None], np.full(n, r), trace))
    return [np.concatenate(z) for z in zip(*out)]


@pytest.mark.parametrize("nc", [3, 4, 5, 6])
def test_mixn_state_functions_at_trace_density(amd, oracle, mix, totals, nc):
    """The n-component path with one or two components at trace or zero density against mixn_derivatives(prec=1), tolerances of
    tests/test_mixn_gpu.py::test_random_rows_vs_oracle; mu and v of a trace component at 1e-300 equal those at 0 to 1e-14."""
    P2, _, T2, _ = mix
    rows0, tot = totals
    keep = np.nonzero(rows0 % 6 <= 2)[0][:60]
    rng = np.random.default_rng(50 + nc)
    P, T, rho, q, trace = _mixn_states(P2[rows0[keep]], T2[rows0[keep]], tot[0, 0, keep], tot[1, 0, keep], nc, rng)
    a, p, mu, v = (_np(x) for x in amd.PcSaftMix(_d(P)).derivatives(_d(T), _d(rho)))
    assert all(np.all(np.isfinite(x)) for x in (a, p, mu, v))
    A, Pp, MU, V = oracle.mixn_derivatives(P, T, rho, prec=1)
    _report(f"nc = {nc}", _errors(a, p, mu, v, A, Pp, MU, V, rho), q, (1e-12, 1e-11, 1e-12, 1e-9))
    n = len(keep)
    blocks = lambda x: x.reshape(2, len(TRACE_RATIOS), n, nc)
    M, Vv, Tr = blocks(mu), blocks(v), blocks(trace)
    dm = np.abs(M[:, 1] - M[:, 0])[Tr[:, 0]] / np.maximum(1.0, np.abs(M[:, 0][Tr[:, 0]]))
    dv = np.abs(Vv[:, 1] / Vv[:, 0] - 1.0)[Tr[:, 0]]
    print(f"   infinite dilution (1e-300 vs 0): mu {dm.max():.2e}, v {dv.max():.2e} (tol 1e-14)")
    assert dm.max() < 1e-14 and dv.max() < 1e-14


@pytest.mark.parametrize("nc", [3, 4, 5, 6])
def test_mixn_backward_at_trace_density(amd, oracle, mix, totals, nc):
    """pcs_mixn_derivatives_vjp (through autograd) at the trace densities (zero included) of test_mixn_state_functions_at_trace_density:
    finite, and against long-double central differences (tolerance of
    tests/test_mixn_gpu.py::test_vjp_vs_finite_differences_of_the_oracle)."""
    P2, _, T2, _ = mix
    rows0, tot = totals
    keep = np.nonzero(rows0 % 6 <= 2)[0][:60]
    rng = np.random.default_rng(50 + nc)
    P, T, rho, q, trace = _mixn_states(P2[rows0[keep]], T2[rows0[keep]], tot[0, 0, keep], tot[1, 0, keep], nc, rng)
    n = len(keep)
    sub = np.arange(0, len(T), n)[:, None] + np.arange(4)[None, :]  # four rows of every (phase, ratio) block
    sub = sub.ravel()
    Ps, Ts, rs = P[sub], T[sub], rho[sub]
    m = len(sub)
    ga, gp, gmu, gv = rng.normal(size=m), rng.normal(size=m), rng.normal(size=(m, nc)), rng.normal(size=(m, nc)) * 1e-3
    par, temp, den = (_d(x).requires_grad_(True) for x in (Ps, Ts, rs))
    a_, p_, mu_, v_ = amd.PcSaftMix(par).derivatives(temp, den)
    ((a_ * _d(ga)).sum() + (p_ * _d(gp)).sum() + (mu_ * _d(gmu)).sum() + (v_ * _d(gv)).sum()).backward()
    g = np.concatenate([_np(par.grad).reshape(m, 8 * nc), _np(temp.grad)[:, None], _np(den.grad)], axis=1)
    X = np.concatenate([Ps.reshape(m, 8 * nc), Ts[:, None], rs], axis=1)

    def L(X_):
        A_, P_, MU_, V_ = oracle.mixn_derivatives(X_[:, :8 * nc].reshape(m, nc, 8), X_[:, 8 * nc], X_[:, 8 * nc + 1:], prec=1)
        return ga * A_ + gp * P_ + (gmu * MU_).sum(axis=1) + (gv * V_).sum(axis=1)

    skip = {8 * c + k for c in range(nc) for k in (6, 7)}
    err = _fd_check(g, X, L, skip=skip, rho_cols=set(range(8 * nc + 1, 9 * nc + 1)), tot=rs.sum(axis=1))
    print(f"   backward vs long-double central differences on {m} states: {err:.2e} (tol 2e-4)")
    assert err < 2e-4


def test_gc_state_functions_at_trace_density(amd, oracle, table, gc_grid):
    """GcPcSaftMix.derivatives at trace partial densities against the oracle (tolerances of the n-component test, the gc oracle
    being a restatement in double precision); infinite dilution to 1e-14."""
    g = gc_grid
    G = len(DILUTE_Z)
    j0, j1 = DILUTE_Z.index(2.0**-20), DILUTE_Z.index(1.0 - 2.0**-20)
    _, rho4, st = g["ref"][False]
    base = np.array([r * G + j0 for r in range(N_GC) if not st[r * G + j0] and not st[r * G + j1]][:60])
    b1 = base - j0 + j1
    tot = np.array([[rho4[base, 0:2].sum(axis=1), rho4[b1, 0:2].sum(axis=1)], [rho4[base, 2:4].sum(axis=1), rho4[b1, 2:4].sum(axis=1)]])
    idx, rho, q, _ = _trace_states(tot)
    rows = base[idx]
    segs, bonds = [g["segs"][r] for r in rows], [g["bonds"][r] for r in rows]
    phi, T = g["phi"][rows], g["T"][rows]
    eos, _ = _gc_model(amd, table, segs, bonds, g["kab_list"], torch.tensor(phi, dtype=f64))
    a, p, mu, v = (_np(x) for x in eos.derivatives(torch.tensor(T, dtype=f64), torch.tensor(rho, dtype=f64)))
    assert all(np.all(np.isfinite(x)) for x in (a, p, mu, v))
    enc = oracle.gc_encode(table, segs, bonds, g["kab_list"])
    A, Pp, MU, V = oracle.gc_derivatives(enc, phi, T, rho, robust=True)
    _report("gc", _errors(a, p, mu, v, A, Pp, MU, V, rho), q, (1e-12, 1e-11, 1e-12, 1e-9))
    dm, dv = _dilution(mu, v, len(base))
    print(f"   infinite dilution (1e-300 vs 0): mu {dm[1]:.2e}, v {dv[1]:.2e} (tol 1e-14)")
    assert dm[1] < 1e-14 and dv[1] < 1e-14


def test_gc_backward_at_trace_density(amd, oracle, table, gc_grid):
    """pcs_gc_derivatives_vjp (through autograd, in phi, T and the densities) at the trace densities (zero included) of
    test_gc_state_functions_at_trace_density: finite, and against central differences of the oracle."""
    g = gc_grid
    G = len(DILUTE_Z)
    j0, j1 = DILUTE_Z.index(2.0**-20), DILUTE_Z.index(1.0 - 2.0**-20)
    _, rho4, st = g["ref"][False]
    base = np.array([r * G + j0 for r in range(N_GC) if not st[r * G + j0] and not st[r * G + j1]][:60])
    b1 = base - j0 + j1
    tot = np.array([[rho4[base, 0:2].sum(axis=1), rho4[b1, 0:2].sum(axis=1)], [rho4[base, 2:4].sum(axis=1), rho4[b1, 2:4].sum(axis=1)]])
    idx, rho, q, _ = _trace_states(tot)
    rows = base[idx]
    segs, bonds = [g["segs"][r] for r in rows], [g["bonds"][r] for r in rows]
    phi, T = g["phi"][rows], g["T"][rows]
    sub = np.nonzero(np.isin(idx, np.arange(6)))[0]
    m = len(sub)
    rng = np.random.default_rng(4)
    ga, gp, gmu, gv = rng.normal(size=m), rng.normal(size=m), rng.normal(size=(m, 2)), rng.normal(size=(m, 2)) * 1e-3
    ph = torch.tensor(phi[sub], dtype=f64, requires_grad=True)
    temp = torch.tensor(T[sub], dtype=f64, requires_grad=True)
    den = torch.tensor(rho[sub], dtype=f64, requires_grad=True)
    segs_s, bonds_s = [segs[k] for k in sub], [bonds[k] for k in sub]
    eos_s, _ = _gc_model(amd, table, segs_s, bonds_s, g["kab_list"], ph)
    a_, p_, mu_, v_ = eos_s.derivatives(temp, den)
    t = lambda x: torch.tensor(x, dtype=f64).to(a_.device)
    ((a_ * t(ga)).sum() + (p_ * t(gp)).sum() + (mu_ * t(gmu)).sum() + (v_ * t(gv)).sum()).backward()
    gr = np.concatenate([_np(ph.grad), _np(temp.grad)[:, None], _np(den.grad)], axis=1)
    X = np.concatenate([phi[sub], T[sub, None], rho[sub]], axis=1)
    enc_s = oracle.gc_encode(table, segs_s, bonds_s, g["kab_list"])

    def L(X_):
        A_, P_, MU_, V_ = oracle.gc_derivatives(enc_s, X_[:, 0:2], X_[:, 2], X_[:, 3:5], robust=True)
        return ga * A_ + gp * P_ + (gmu * MU_).sum(axis=1) + (gv * V_).sum(axis=1)

    err = _fd_check(gr, X, L, skip=set(), rho_cols={3, 4}, tot=rho[sub].sum(axis=1))
    print(f"   backward (phi, T, rho) vs central differences on {m} states: {err:.2e} (tol 2e-4)")
    assert err < 2e-4


# ---------------------------------------------------------------------------------------------------------------------------
# stability at dilute feeds
# ---------------------------------------------------------------------------------------------------------------------------
TPD_TOL = 1e-8


def test_stability_at_dilute_feeds(oracle, mix, mix_solved):
    """pcs_mix_stability on the specified phases of converged dilute rows (100 bubble liquids, 100 dew vapours, all z of the
    grid) against the brute-force referee, whose trial compositions reach down to 1e-14 on either side; the rules of
    tests/test_stability_gpu.py::test_referee_agreement.  A feed with a zero partial density is invalid (status 3)."""
    from feos_torch_amd import native

    P, K, T, _ = mix
    feeds, rows = [], []
    for dew in (False, True):
        m = mix_solved[dew]
        okk = np.argwhere(~m["st"][:, :len(DILUTE_Z)])
        sel = okk[np.linspace(0, len(okk) - 1, 100).astype(np.int64)]
        r4 = m["rho4"][sel[:, 0], sel[:, 1]]
        feeds.append(r4[:, 0:2] if dew else r4[:, 2:4])
        rows.append(sel[:, 0])
    feed, rows = np.concatenate(feeds), np.concatenate(rows)
    Pk, Kk, Tk = P[rows], K[rows], T[rows]
    r = native.mix_stability(_d(Pk), _d(Kk), _d(Tk), _d(feed))
    s, tpd, tr = _np(r["status"]), _np(r["tpd"]), _np(r["rho_trial"])
    d = R.mix_derivs(oracle, Pk, Kk, Tk)
    lo = np.logspace(-14, -8, 13)
    extra = np.broadcast_to(np.concatenate([lo, 1.0 - lo])[None, :], (len(feed), 26))
    ref = R.tpd_minimum(d, R.mix_packing(Pk, Tk), feed, extra_w=extra)
    noise = R.mix_pressure_noise(oracle, Pk, Kk, Tk, feed)
    judged = noise <= 1e-6 * np.abs(ref["pf"])
    rt = ref["tpd"]
    print(f"{len(feed)} dilute feeds, {judged.sum()} judged; kernel status counts {np.bincount(s, minlength=4)}; referee < -1e-5 on "
          f"{(rt < -1e-5).sum()}; kernel unstable / referee within 1e-5 of 0 on {((rt >= -1e-5) & (s != 0) & judged).sum()}")
    assert np.all(s[judged & (rt < -1e-5)] != 0)
    assert np.all(rt[judged & (s == 0)] >= -1e-5)
    # status 3: p^f <= 0 -- a liquid at ~1e-16 A^-3 whose fp64 pressure is below its own rounding; never a judged feed
    assert not np.any(judged[s == 3]) and np.all(ref["pf"][s == 3] <= noise[s == 3])
    u = np.nonzero(s == 1)[0]
    if len(u):
        nz = R.mix_pressure_noise(oracle, Pk[u], Kk[u], Tk[u], feed[u]) + R.mix_pressure_noise(oracle, Pk[u], Kk[u], Tk[u], tr[u])
        pf, _, t_cpu = R.recompute(d, u, feed[u], tr[u])
        assert np.all(R.is_root(d, u, pf, tr[u], nz))
        assert np.all(np.abs(t_cpu - tpd[u]) <= 1e-9 + 2.0 * nz / tr[u].sum(axis=1))
        assert np.all(t_cpu < -TPD_TOL)
    tot = feed.sum(axis=1)[:4]
    zero = np.array([[0.0, tot[0]], [tot[1], 0.0], [0.0, tot[2]], [tot[3], 0.0]])
    r0 = native.mix_stability(_d(Pk[:4]), _d(Kk[:4]), _d(Tk[:4]), _d(zero))
    assert np.all(_np(r0["status"]) == 3) and np.all(np.isnan(_np(r0["tpd"])))
