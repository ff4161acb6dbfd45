"""CPU: the exact-gradient referees of the binary and pure state-function backward kernels, checked by the oracle alone.

oracle.mix_derivatives_vjp_exact  (derivatives_mix over DualN<long double, 21>: 16 parameters, k_ij, eps_AiBj, T, rho_0, rho_1)
oracle.pure_derivatives_vjp_exact (derivatives over DualN<long double, 10>: 8 parameters, T, rho)
are what tests/test_mix_state_gpu.py and tests/test_pure_state_gpu.py hold pcs_mix_derivatives_vjp and pcs_pure_derivatives_vjp
to.  Here they are tied to
  * Richardson-extrapolated central differences of the long-double forward evaluation, every column with a value to step;
  * the density identities mu_i = da/drho_i (binary) and dp/drho of the forward = the rho column of L = p (pure);
  * the n-component referee (oracle/pcsaft_mixn.hpp, written separately) at nc = 2, k_ij = 0, and at nc = 1;
  * the unmodified reference's own autograd on its test inputs (tests/golden/deriv_grad.json), which fixes the structural-zero
    and site-count conventions.
Rows: tests/tools/state_rows.py (the rows of the GPU tests)."""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import state_rows as sr  # noqa: E402

STEPS = (1e-5, 5e-6)  # relative steps, as tests/test_oracle_mixn.py
U = 1.1e-16


def _richardson(L, X, skip):
    """Central differences of L(X) [n] at the two relative steps per column of X [n, k]: (extrapolated value, |d(h1) - d(h2)|).
    Entries in `skip` (nothing to step: the value is 0) are not differenced and come back as 0."""
    fd, spread = np.zeros_like(X), np.zeros_like(X)
    for k in range(X.shape[1]):
        d, w2 = [], []
        for s in STEPS:
            h = np.where(skip[:, k], 0.0, s * np.abs(X[:, k]))
            Xp, Xm = X.copy(), X.copy()
            Xp[:, k] += h
            Xm[:, k] -= h
            width = np.where(skip[:, k], 1.0, Xp[:, k] - Xm[:, k])  # the step actually taken
            d.append((L(Xp) - L(Xm)) / width)
            w2.append(width**2)
        fd[:, k] = np.where(skip[:, k], 0.0, (w2[0] * d[1] - w2[1] * d[0]) / np.where(skip[:, k], 1.0, w2[0] - w2[1]))
        spread[:, k] = np.abs(d[0] - d[1])
    return fd, spread


def _check_richardson(label, g, fd, spread, X, skip, tsum, q90=1e-8):
    """Measure and bars of tests/test_oracle_mixn.py::test_exact_gradient_vs_richardson_differences: the log-derivative
    |x_k| |g_k - fd_k| / max_j |x_j g_j| per row; bar per entry = rounding 12 u Tsum / (s1 max|x g|) (the forward outputs are
    rounded to double and L is summed in double: |dL| <= 4 u Tsum; two evaluations per difference over a width 2 s x, weights
    4/3 and 1/3) + truncation |x| |d(h1) - d(h2)| / max|x g| (the whole h^2 term the extrapolation removes).  So that the
    per-entry bar hides nothing: nine rows in ten have every bar below q90 = 1e-8, and the median row agrees to 1e-9 whatever
    its bar."""
    sc = np.abs(X)
    lg = np.where(skip, 0.0, sc * np.abs(g)).max(axis=1, keepdims=True)
    err = np.where(skip, 0.0, sc * np.abs(g - fd)) / lg
    bar = 12 * U / STEPS[0] * tsum[:, None] / lg + sc * spread / lg
    row_bar = np.where(skip, 0.0, bar).max(axis=1)
    ratio = np.where(skip | (err == 0.0), 0.0, err / np.where(bar == 0.0, 1.0, bar))
    print(f"{label}: columns compared {int((~skip).any(axis=0).sum())}, max err {err.max():.2e}, median row {np.median(err.max(axis=1)):.2e}, "
          f"max err / bar {ratio.max():.2f}, row bar quantiles 0.5 / 0.9 / 1: {np.quantile(row_bar, [0.5, 0.9, 1.0])}")
    assert np.quantile(row_bar, 0.9) < q90
    assert np.median(err.max(axis=1)) < 1e-9
    assert (err <= bar).all(), ratio.max()


@pytest.mark.parametrize("state", sr.STATES)
def test_mix_exact_gradient_vs_richardson_differences(oracle, state):
    """Every column of the binary referee whose input is non-zero (all of m, sigma, epsilon_k, k_ij, T, rho; mu, kappa_ab,
    epsilon_k_ab, na, nb and eps_AiBj where the row has them), the first 120 rows (20 of each class of mix_batch) of each state.
    A zero-valued input has no relative step; its column is tied to the reference's autograd by the fixture test below.
    Measured, vapour / liquid / compressed: largest error 1.1e-9 / 4.8e-11 / 1.5e-11, median over the rows 3.4e-11 / 5.7e-12 /
    6.9e-13; largest error / bar 0.35 / 0.36 / 0.35; row bar 0.9 quantile 6.6e-10 / 3.5e-9 / 2.3e-9."""
    m = sr.mix_rows(oracle)
    n = 120
    P, K, T, rho = m["P"][:n], m["K"][:n], m["T"][:n], m["states"][state][:n]
    ga, gp, gmu, gv = (x[:n] for x in m["w"][state])
    g = m["exact"][state][:n]
    X = np.concatenate([P.reshape(n, 16), K, T[:, None], rho], axis=1)
    skip = X == 0.0
    assert all((~skip[:, k]).any() for k in range(21))  # every one of the 21 columns is differenced on some row

    def L(Z):
        a, p, mu, v = oracle.mix_derivatives_exact(Z[:, :16].reshape(n, 2, 8), Z[:, 16:18], Z[:, 18], Z[:, 19:21])
        return ga * a + gp * p + (gmu * mu).sum(axis=1) + (gv * v).sum(axis=1)

    fd, spread = _richardson(L, X, skip)
    a, p, mu, v = oracle.mix_derivatives_exact(P, K, T, rho)
    tsum = np.abs(ga * a) + np.abs(gp * p) + np.abs(gmu * mu).sum(axis=1) + np.abs(gv * v).sum(axis=1)
    _check_richardson(f"binary {state}", g, fd, spread, X, skip, tsum)


@pytest.mark.parametrize("state", sr.STATES)
def test_pure_exact_gradient_vs_richardson_differences(oracle, state):
    """Every column of the pure referee whose input is non-zero, the first 200 rows of each state, L = ga a + gp p + gdp dp/drho.
    Measured, vapour / liquid / compressed: largest error 5.2e-8 / 2.0e-12 / 2.9e-12, median over the rows 1.3e-10 / 1.0e-12 /
    1.3e-12; largest error / bar 0.33 / 0.33 / 0.28; row bar 0.9 quantile 1.02e-8 / 3.1e-9 / 2.6e-9."""
    q = sr.pure_rows(oracle)
    n = 200
    P, T, rho = q["P"][:n], q["T"][:n], q["states"][state][:n]
    ga, gp, gdp = (x[:n] for x in q["w"][state])
    g = q["exact"][state][:n]
    X = np.concatenate([P, T[:, None], rho[:, None]], axis=1)
    skip = X == 0.0
    assert all((~skip[:, k]).any() for k in range(10))

    def L(Z):
        a, p, dp = oracle.pure_derivatives(Z[:, :8], Z[:, 8], Z[:, 9], prec=1)
        return ga * a + gp * p + gdp * dp

    fd, spread = _richardson(L, X, skip)
    a, p, dp = oracle.pure_derivatives(P, T, rho, prec=1)
    tsum = np.abs(ga * a) + np.abs(gp * p) + np.abs(gdp * dp)
    # vapour: dp/drho = 1 + O(rho), so gdp dp is of size 1 and makes up Tsum, while every x dL/dx is O(rho B): Tsum / max|x g| is
    # 100 and more on one gas row in five, and the rounding term 1.3e-10 Tsum / max|x g| alone passes 1e-8 there
    _check_richardson(f"pure {state}", g, fd, spread, X, skip, tsum, q90=3e-8 if state == "vapour" else 1e-8)


def test_density_identities(oracle):
    """Binary, L = a: dL/drho_i = mu_i, the DualN tangent against the eps1 part of the HyperDual.  Pure, L = p: dL/drho = the
    dp/drho output of the forward, the DualN tangent against the v2 part of the Dual3.  Both sides long double in everything and
    rounded to double once: 1e-15 max(1, |.|) (the bar of the nc = 2 check in tests/test_oracle_mixn.py).  All rows, all states.
    Measured: 1.4e-16 (binary), 2.1e-16 (pure)."""
    m = sr.mix_rows(oracle)
    n = m["n"]
    z = np.zeros((n, 2))
    for state, rho in m["states"].items():
        g = oracle.mix_derivatives_vjp_exact(m["P"], m["K"], m["T"], rho, np.ones(n), np.zeros(n), z, z, prec=1)
        _, _, mu, _ = oracle.mix_derivatives_exact(m["P"], m["K"], m["T"], rho)
        d = np.abs(g[:, 19:21] - mu) / np.maximum(1.0, np.abs(mu))
        print(f"binary {state}: max |da/drho - mu| / max(1, |mu|) = {d.max():.2e}")
        assert d.max() < 1e-15
    q = sr.pure_rows(oracle)
    n = q["n"]
    for state, rho in q["states"].items():
        g = oracle.pure_derivatives_vjp_exact(q["P"], q["T"], rho, np.zeros(n), np.ones(n), np.zeros(n), prec=1)
        _, _, dp = oracle.pure_derivatives(q["P"], q["T"], rho, prec=1)
        d = np.abs(g[:, 9] - dp) / np.maximum(1.0, np.abs(dp))
        print(f"pure {state}: max |d p/d rho - dp| / max(1, |dp|) = {d.max():.2e}")
        assert d.max() < 1e-15


def _spread_bar(a1, a0, b1, b0, groups, model=0.0):
    """Bar of a comparison of two long-double referees a1, b1 that compute the same function by different code: per row and
    group, the prec=0 against prec=1 spread of either (how far an fp64 evaluation of each formula is from its long-double one:
    the conditioning of the row) plus 4 u for the two roundings to double on return plus `model`, the allowance for constants
    that the two codes form differently in double."""
    ea, eb = sr.group_error(a0, a1, groups), sr.group_error(b0, b1, groups)
    return {g: ea[g] + eb[g] + 4 * U + model for g in groups}


def test_mix_exact_gradient_equals_the_n_component_referee(oracle):
    """k_ij = 0 and at most one associating component: the binary model is the n-component one at nc = 2 (oracle/pcsaft_mixn.hpp,
    written separately: its own dispersion and dipole sums, its own association code).  Columns 0:16 and 18:21 of the binary
    referee against mixn_derivatives_vjp_exact, all 350 such rows of the row set, three states, per input group.
    Measured: largest difference 2.2e-16, at most 0.03 of its bar; bar median 1e-15 ... 8e-15."""
    m = sr.mix_rows(oracle)
    rows = np.nonzero(m["classes"]["none"] | m["classes"]["one"])[0]
    assert len(rows) >= 300 and m["classes"]["one"][rows].sum() >= 100
    P, T = np.ascontiguousarray(m["P"][rows]), np.ascontiguousarray(m["T"][rows])
    K = np.zeros((len(rows), 2))
    groups = {"parameters": slice(0, 16), "T": slice(16, 17), "rho": slice(17, 19)}
    cols = list(range(16)) + [18, 19, 20]
    for state in sr.STATES:
        rho = np.ascontiguousarray(m["states"][state][rows])
        w = [np.ascontiguousarray(x[rows]) for x in m["w"][state]]
        b1, b0 = (oracle.mix_derivatives_vjp_exact(P, K, T, rho, *w, prec=k) for k in (1, 0))
        assert np.all(b1[:, 16:18][:, 1] == 0.0)  # eps_AiBj: not a cross-associating row
        n1, n0 = (oracle.mixn_derivatives_vjp_exact(P, T, rho, *w, prec=k) for k in (1, 0))
        err = sr.group_error(b1[:, cols], n1, groups)
        bar = _spread_bar(b1[:, cols], b0[:, cols], n1, n0, groups)
        for g in groups:
            print(f"binary vs nc = 2, {state} {g}: max difference {err[g].max():.2e}, max difference / bar {np.max(err[g] / bar[g]):.2f}, "
                  f"bar median {np.median(bar[g]):.1e} max {bar[g].max():.1e}")
            assert np.median(bar[g]) < 1e-13 and (err[g] <= bar[g]).all(), (state, g)


def test_pure_exact_gradient_equals_the_n_component_referee(oracle):
    """nc = 1 of the n-component model is the pure model (other formulas: the dipole term with mu^2 not factored out, the
    mixture's association strength).  L = ga a + gp p (the mixture has no dp/drho output; mu and v of one component are
    (p - rho + a) / rho and 1 / rho); all 10 columns, all rows, three states.
    The two codes are not the same function to the last bit even in long double: both form pi / 6 in double before it meets a
    long double, and the mixture code also 6 / pi for its hard-sphere term where the pure code has none (found with a
    150-digit mpmath evaluation of one liquid row: the long-double dp/drho of either code is 7e-16 from the exact value of the
    formulas with exact quotients, the fp64 one no further).  Two constants off by u = 1.1e-16 each, log-sensitivities of the
    liquid gradients to the packing fraction up to 100 (the hard-sphere and dispersion parts of rho a'' are 10 to 100 times
    their sum): `model` = 2 * 100 u = 2.2e-14, the size of the 2e-14 that tests/test_oracle_mixn.py allows for the same reason.
    Measured: largest difference 3.2e-13 (a liquid row with a wide spread); largest difference / bar 0.25; bar median 2.7e-14."""
    q = sr.pure_rows(oracle)
    n = q["n"]
    z = np.zeros((n, 1))
    for state, rho in q["states"].items():
        ga, gp, _ = q["w"][state]
        p1, p0 = (oracle.pure_derivatives_vjp_exact(q["P"], q["T"], rho, ga, gp, np.zeros(n), prec=k) for k in (1, 0))
        n1, n0 = (oracle.mixn_derivatives_vjp_exact(q["P"][:, None, :], q["T"], rho[:, None], ga, gp, z, z, prec=k) for k in (1, 0))
        err = sr.group_error(p1, n1, sr.PURE_GROUPS)
        bar = _spread_bar(p1, p0, n1, n0, sr.PURE_GROUPS, model=200 * U)
        for g in sr.PURE_GROUPS:
            print(f"pure vs nc = 1, {state} {g}: max difference {err[g].max():.2e}, max difference / bar {np.max(err[g] / bar[g]):.2f}, "
                  f"bar median {np.median(bar[g]):.1e} max {bar[g].max():.1e}")
            assert np.median(bar[g]) < 1e-13 and (err[g] <= bar[g]).all(), (state, g)


def _rows_close(got, ref, tol):
    """tests/test_deriv_grad_gpu.py::rows_close"""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    got, ref = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    err = np.max(np.abs(got - ref), axis=1) / np.maximum(np.max(np.abs(ref), axis=1), 1e-300)
    assert (err <= tol).all(), (np.nonzero(err > tol)[0][:5], err.max())
    return err.max()


def test_referees_vs_reference_autograd(oracle):
    """The reference's own fp64 autograd on its test inputs (tests/golden/deriv_grad.json: the 14 binary cases of every
    association class, 12 pure cases), per input at the tolerances tests/test_deriv_grad_gpu.py holds the kernels to: 1e-7
    for parameters and kij, 1e-8 (binary) / 1e-9 (pure) for T and rho.  The zero pattern is the reference's: the eps_AiBj
    column is 0 except on the cross-associating case with an explicit value, the mu column 0 where mu = 0."""
    g = load_golden("deriv_grad.json")["mix"]["test_inputs"]
    P, K, T, rho, w = (np.array(g[k]) for k in ("params", "kij", "T", "rho", "w"))
    got = oracle.mix_derivatives_vjp_exact(P, K, T, rho, w[0], w[1], w[2:4].T.copy(), w[4:6].T.copy(), prec=1)
    e = [_rows_close(got[:, 0:16], g["grad_params"], 1e-7), _rows_close(got[:, 16:18], g["grad_kij"], 1e-7),
         _rows_close(got[:, 18:19], np.array(g["grad_T"])[:, None], 1e-8), _rows_close(got[:, 19:21], g["grad_rho"], 1e-8)]
    print("binary referee vs reference autograd (parameters, kij, T, rho):", " ".join(f"{x:.2e}" for x in e))
    ref_k, ref_p = np.array(g["grad_kij"]), np.array(g["grad_params"]).reshape(len(T), 16)
    assert np.array_equal(got[:, 17] != 0.0, ref_k[:, 1] != 0.0) and (ref_k[:, 1] != 0.0).sum() == 1
    assert np.array_equal(got[:, 0:16] == 0.0, ref_p == 0.0)
    g = load_golden("deriv_grad.json")["pure"]["test_inputs"]
    P, T, rho, w = (np.array(g[k]) for k in ("params", "T", "rho", "w"))
    n = len(T)
    for got, ref in ((oracle.pure_derivatives_vjp_exact(P, T, rho, *w, prec=1), g),
                     (oracle.pure_derivatives_vjp_exact(P, T, rho, np.ones(n), np.zeros(n), np.zeros(n), prec=1), g["a_only"])):
        e = [_rows_close(got[:, 0:8], ref["grad_params"], 1e-7), _rows_close(got[:, 8:9], np.array(ref["grad_T"])[:, None], 1e-9),
             _rows_close(got[:, 9:10], np.array(ref["grad_rho"])[:, None], 1e-9)]
        print("pure referee vs reference autograd (parameters, T, rho):", " ".join(f"{x:.2e}" for x in e))
        # (one way only: the reference's kappa_ab entry of the case with B sites alone, where X_B = 1 identically, is 1.5e-17 of
        # rounding; the long-double site fractions give the exact 0)
        assert np.all(got[:, 0:8][np.array(ref["grad_params"]) == 0.0] == 0.0)


def test_pure_forward_long_double_and_fp64_paths(oracle):
    """pure_derivatives(prec=1) is the long-double evaluation (the fp64 one stays within its own rounding of it on rows without
    strong association, and is not the same number), and prec=0 is still the default path."""
    q = sr.pure_rows(oracle)
    rho = q["states"]["liquid"]
    d0, dd, d1 = oracle.pure_derivatives(q["P"], q["T"], rho), oracle.pure_derivatives(q["P"], q["T"], rho, prec=0), \
        oracle.pure_derivatives(q["P"], q["T"], rho, prec=1)
    assert all(np.array_equal(x, y) for x, y in zip(d0, dd))
    assert any(not np.array_equal(x, y) for x, y in zip(d0, d1))
    plain = q["P"][:, 6] == 0.0
    assert np.max(np.abs(d0[0] - d1[0])[plain] / np.abs(d1[0][plain])) < 1e-13
