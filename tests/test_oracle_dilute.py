"""CPU: the long-double references in the dilute limit, before the GPU is held to them (tests/test_dilute_gpu.py).

Every other mixture test draws its compositions from [0.1, 0.9].  Here seeded rows are solved with a trace amount of either
component, z in DILUTE_Z (tests/tools/dilute_grid.py), and the oracle's bubble / dew solver (oracle/mix_solver.hpp, which
mirrors the kernels decision by decision) is checked against judges that do not share its decisions:
  * the continuation solver (oracle/mix_continuation.hpp, a second, independent solver), wherever it returns a solution;
  * the phase-equilibrium conditions in the long-double state functions (equal ln rho_i + mu_i, equal p);
  * the pure-component limit: the vapour pressure of the component that remains, in the Henry-linear form p = p_sat + s d.
gc rows have no second solver: there the fp64 and the long-double solver and the equilibrium conditions are the judges."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
from dilute_grid import DILUTE_Z, KT_A3, grid, henry_error, trace_fraction_error  # noqa: E402

N_MIX = 600
N_GC = 400


@pytest.fixture(scope="module")
def mix_rows():
    from feos_torch_amd.synthetic import mix_batch

    return mix_batch(N_MIX, seed=91)


@pytest.fixture(scope="module")
def mix_solved(oracle, mix_rows):
    """{dew: (p [N_MIX, G], rho4 [N_MIX, G, 4], status [N_MIX, G])}"""
    P, K, T, _, PI = mix_rows
    G = len(DILUTE_Z)
    i, z = grid(N_MIX, DILUTE_Z)
    out = {}
    for dew in (False, True):
        p, rho4, st = oracle.mix_bubble_dew(P[i], K[i], T[i], z, PI[i], dew, prec=1)
        out[dew] = (p.reshape(N_MIX, G), rho4.reshape(N_MIX, G, 4), st.reshape(N_MIX, G))
    return out


def test_exact_pure_compositions_fail(oracle, mix_rows):
    """z = 0 and z = 1 have no solution in the solver's formulation (include/pcsaft_hip.h: 0 < z < 1)."""
    P, K, T, _, PI = mix_rows
    n = 60
    for dew in (False, True):
        for z in (0.0, 1.0):
            _, _, st = oracle.mix_bubble_dew(P[:n], K[:n], T[:n], np.full(n, z), PI[:n], dew, prec=1)
            assert st.all(), (dew, z, int((~st).sum()))


@pytest.mark.parametrize("dew", [False, True])
def test_mix_converges_and_meets_equilibrium(oracle, mix_rows, mix_solved, dew):
    """Residuals of the equilibrium conditions with the tolerances of
    tests/test_mix_gpu.py::test_phase_equilibrium_conditions_large_batch (q99.9 there, q99 on this smaller sample; p of the
    vapour, as there); the
    specified phase keeps the specified trace fraction to 1e-12 of itself."""
    P, K, T, _, _ = mix_rows
    p, rho4, st = mix_solved[dew]
    conv = (~st).sum(axis=0)
    print(f"{'dew' if dew else 'bubble'}: converged rows per z {conv.tolist()} of {N_MIX}")
    assert np.all(conv >= 0.98 * N_MIX)
    worst = np.zeros(3)
    for j, zz in enumerate(DILUTE_Z):
        ok = ~st[:, j]
        r = rho4[ok, j]
        _, pV, muV, _ = oracle.mix_derivatives_exact(P[ok], K[ok], T[ok], r[:, 0:2])
        _, _, muL, _ = oracle.mix_derivatives_exact(P[ok], K[ok], T[ok], r[:, 2:4])
        dmu = np.abs(np.log(r[:, 0:2]) + muV - np.log(r[:, 2:4]) - muL).max(axis=1)
        pr = p[ok, j] / (KT_A3 * T[ok])
        dp = np.abs(pV / pr - 1)  # the liquid's pressure is a difference of O(rho_L) terms: not determined relative to p
        dz = trace_fraction_error(r[:, 0:2] if dew else r[:, 2:4], np.full(ok.sum(), zz))
        q = np.array([np.quantile(dmu, 0.99), np.quantile(dp, 0.99), dz.max()])
        print(f"   z = {zz:.6g}: |d ln f| q99 {q[0]:.2e} max {dmu.max():.2e}; |dp/p| q99 {q[1]:.2e} max {dp.max():.2e}; "
              f"trace fraction {q[2]:.2e}")
        # the stagnation exit (Newton step < 1e-7 but no longer shrinking) leaves a handful of rows with a larger residual
        assert dmu.max() < 1e-3 and (dmu > 1e-6).sum() <= 2
        assert dp.max() < 1e-4 and (dp > 1e-6).sum() <= 2
        assert q[0] < 1e-10 and q[1] < 1e-9 and q[2] < 1e-12
        worst = np.maximum(worst, q)
    print(f"   worst: |d ln f| {worst[0]:.2e} (tol 1e-10), |dp/p| {worst[1]:.2e} (tol 1e-9), trace fraction {worst[2]:.2e} (tol 1e-12)")


@pytest.mark.parametrize("dew", [False, True])
def test_mix_vs_continuation(oracle, mix_rows, mix_solved, dew):
    """The independent continuation solver, wherever it returns a solution (code 0): 1e-9 relative in p (the tolerance of
    tests/test_mix_gpu.py::test_random_batch_vs_oracle).  Rows where the two land on different solutions may be at most 1 %."""
    P, K, T, _, _ = mix_rows
    p, _, st = mix_solved[dew]
    worst, n_cmp, n_diff = 0.0, 0, 0
    for j, zz in enumerate(DILUTE_Z):
        pc, _, code, _ = oracle.mix_bubble_dew_continuation(P, K, T, np.full(N_MIX, zz), dew)
        both = (code == 0) & ~st[:, j]
        err = np.abs(p[both, j] / pc[both] - 1)
        n_cmp += int(both.sum())
        n_diff += int((err > 1e-9).sum())
        worst = max(worst, float(np.max(err[err <= 1e-9], initial=0.0)))
        assert ((code == 0) & st[:, j]).sum() <= 0.02 * N_MIX, zz  # solutions the oracle misses
    print(f"{'dew' if dew else 'bubble'}: {n_cmp} rows compared, {n_diff} on a different solution; max relative difference "
          f"elsewhere {worst:.2e} (tol 1e-9)")
    assert n_cmp >= 0.8 * N_MIX * len(DILUTE_Z)
    assert n_diff <= 0.01 * n_cmp


@pytest.mark.parametrize("dew", [False, True])
def test_mix_pure_component_limit(oracle, mix_rows, mix_solved, dew):
    """z -> 0: p -> p_sat of component 2; z -> 1: p -> p_sat of component 1 (bubble and dew alike).  Tolerance 1e-9 relative,
    that of p itself."""
    P, K, T, _, _ = mix_rows
    p, _, st = mix_solved[dew]
    j = {z: i for i, z in enumerate(DILUTE_Z)}
    # (remaining component, columns of d_tiny / d_lo / d_hi, d_tiny, d_lo, d_hi); near z = 1 only two points: d_tiny = d_lo
    sides = ((1, (j[2.0**-46], j[2.0**-30], j[2.0**-20]), 2.0**-46, 2.0**-30, 2.0**-20),
             (0, (j[1 - 2.0**-40], j[1 - 2.0**-40], j[1 - 2.0**-20]), 2.0**-40, 2.0**-40, 2.0**-20))
    for comp, cols, d_tiny, d_lo, d_hi in sides:
        psat, pst = oracle.pure_vapor_pressure(P[:, comp], T, prec=1)
        err, judged = henry_error(p[:, cols[0]], p[:, cols[1]], p[:, cols[2]], d_tiny, d_lo, d_hi, psat)
        ok = ~pst & ~st[:, list(cols)].any(axis=1)
        m = ok & judged
        print(f"{'dew' if dew else 'bubble'}, component {comp + 1} remains: {m.sum()} rows judged ({(ok & ~judged).sum()} not "
              f"Henry-linear), max |p - p_sat - s d| / p_sat {err[m].max():.2e} (tol 1e-9)")
        assert m.sum() >= 0.6 * N_MIX
        assert err[m].max() < 1e-9


@pytest.fixture(scope="module")
def gc_case(oracle):
    from feos_torch_amd.synthetic import gc_batch, load_segment_table

    table = load_segment_table(os.path.join(ROOT, "tests", "data", "sauer2014_hetero.json"))
    b = gc_batch(N_GC, table, seed=93)
    i, z = grid(N_GC, DILUTE_Z)
    enc = oracle.gc_encode(table, [b["segment_lists"][k] for k in i], [b["bond_lists"][k] for k in i], b["kab_list"])
    return b, enc, i, z


@pytest.mark.parametrize("dew", [False, True])
def test_gc_converges_and_meets_equilibrium(oracle, gc_case, dew):
    """gc rows on the dilute grid: the long-double solver converges, fp64 agrees with it, and the equilibrium conditions hold
    in the state functions (tolerances as for the binary rows above)."""
    b, enc, i, z = gc_case
    phi, T, PI = b["phi"][i], b["T"][i], b["p_init"][i]
    p1, rho4, st1 = oracle.gc_bubble_dew(enc, phi, T, z, PI, dew, prec=1)
    p0, _, st0 = oracle.gc_bubble_dew(enc, phi, T, z, PI, dew, prec=0)
    conv = (~st1).reshape(N_GC, -1).sum(axis=0)
    print(f"gc {'dew' if dew else 'bubble'}: converged rows per z {conv.tolist()} of {N_GC}")
    assert np.all(conv >= 0.99 * N_GC)
    assert (st1 != st0).sum() <= 0.005 * len(z)
    both = ~st1 & ~st0
    d64 = np.abs(p0[both] / p1[both] - 1)
    print(f"   fp64 vs long double: max relative difference {d64.max():.2e} (tol 1e-11)")
    assert d64.max() < 1e-11
    ok = ~st1
    r = rho4[ok]
    e = {**enc, "counts": enc["counts"][ok], "bonds": enc["bonds"][ok]}
    _, pV, muV, _ = oracle.gc_derivatives(e, phi[ok], T[ok], r[:, 0:2], robust=True)
    _, _, muL, _ = oracle.gc_derivatives(e, phi[ok], T[ok], r[:, 2:4], robust=True)
    dmu = np.abs(np.log(r[:, 0:2]) + muV - np.log(r[:, 2:4]) - muL).max(axis=1)
    pr = p1[ok] / (KT_A3 * T[ok])
    dp = np.abs(pV / pr - 1)
    dz = trace_fraction_error(r[:, 0:2] if dew else r[:, 2:4], z[ok])
    print(f"   |d ln f| q99 {np.quantile(dmu, 0.99):.2e} max {dmu.max():.2e} (tol 1e-10); |dp/p| q99 {np.quantile(dp, 0.99):.2e} "
          f"max {dp.max():.2e} (tol 1e-9); trace fraction {dz.max():.2e} (tol 1e-12)")
    assert np.quantile(dmu, 0.99) < 1e-10 and np.quantile(dp, 0.99) < 1e-9
    assert (dmu > 1e-6).sum() <= 2 and (dp > 1e-6).sum() <= 2
    assert dz.max() < 1e-12


def test_gc_exact_pure_compositions_fail(oracle, gc_case):
    b, enc, i, _ = gc_case
    n = 40
    rows = np.arange(n) * len(DILUTE_Z)
    e = {**enc, "counts": enc["counts"][rows], "bonds": enc["bonds"][rows]}
    for dew in (False, True):
        for z in (0.0, 1.0):
            _, _, st = oracle.gc_bubble_dew(e, b["phi"][:n], b["T"][:n], np.full(n, z), b["p_init"][:n], dew, prec=1)
            assert st.all(), (dew, z, int((~st).sum()))
