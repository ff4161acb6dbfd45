"""CPU: the oracle's n-component restatement (oracle/pcsaft_mixn.hpp) against the only outputs the unmodified reference can
produce for it (n = 2 with kij = 0, tests/golden/mixn.json; see tests/test_mixn_gpu.py for why) and against exact properties.

The exact gradient (oracle.mixn_derivatives_vjp_exact: nested duals in long double, the referee of the n-component backward
kernel in tests/test_mixn_gpu.py) is checked here by the oracle alone: against Richardson-extrapolated central differences of
the long-double forward evaluation, against mu = da/drho, and at nc = 2 against the binary model's own long-double code."""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
from mixn_rows import random_rows  # noqa: E402


def test_nc2_vs_reference_python(oracle):
    g = load_golden("mixn.json")["nc2_kij0"]
    P, T, rho = (np.array(g[k]) for k in ("params", "T", "rho"))
    a, p, mu, v = oracle.mixn_derivatives(P, T, rho, prec=0)
    assert np.max(np.abs(a - np.array(g["a"]))) < 1e-14
    assert np.max(np.abs(p - np.array(g["p"]))) < 1e-14
    assert np.max(np.abs(mu - np.array(g["mu"]))) < 1e-13
    assert np.max(np.abs(v / np.array(g["v"]) - 1.0)) < 1e-11


def test_splitting_a_component_changes_nothing(oracle):
    g = load_golden("mixn.json")["nc2_kij0"]
    P, T, rho = (np.array(g[k]) for k in ("params", "T", "rho"))
    ok = (P[:, 1, 6] + P[:, 1, 7]) == 0  # the duplicated component must not be the associating one
    a, p, mu, v = oracle.mixn_derivatives(P[ok], T[ok], rho[ok], prec=1)
    P3 = np.concatenate([P, P[:, 1:2, :]], axis=1)[ok]
    rho3 = np.concatenate([rho[:, :1], 0.3 * rho[:, 1:2], 0.7 * rho[:, 1:2]], axis=1)[ok]
    a3, p3, mu3, v3 = oracle.mixn_derivatives(P3, T[ok], rho3, prec=1)
    assert np.max(np.abs(a3 - a)) < 1e-15 and np.max(np.abs(p3 - p)) < 1e-14
    assert np.max(np.abs(mu3[:, :2] - mu)) < 1e-13 and np.max(np.abs(mu3[:, 2] - mu3[:, 1])) < 1e-13
    assert np.max(np.abs(v3[:, :2] / v - 1.0)) < 1e-12


# ---- the exact gradient ------------------------------------------------------------------------------------------------------
TYPICAL = np.array([1.0, 1.0, 1.0, 1.0, 0.01, 2000.0, 1.0, 1.0])  # step scale of a parameter whose value is 0
STEPS = (1e-5, 5e-6)  # relative steps, as orc_gc_derivatives_vjp_exact takes them for the gc segment table


def _weights(n, nc, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=n), rng.normal(size=n), rng.normal(size=(n, nc)), rng.normal(size=(n, nc)) * 1e-3


def _richardson(oracle, P, T, rho, w):
    """Central differences of L = ga a + gp p + gmu . mu + gv . v (oracle.mixn_derivatives, prec=1) at the two steps, per input
    column: (extrapolated value, |d(h1) - d(h2)|, the step scale, the entries not differenced).  A zero-valued parameter is
    stepped by its TYPICAL scale (mu = 0: L is even in mu, both differences are exactly 0).  Not differenced: na, nb of a
    component without sites -- a step there makes a second associating component, another model class."""
    n, nc = rho.shape
    ga, gp, gmu, gv = w
    X = np.concatenate([P.reshape(n, -1), T[:, None], rho], axis=1)
    site_less = np.repeat((P[:, :, 6] + P[:, :, 7]) == 0.0, 8, axis=1) & np.tile(np.arange(8) >= 6, nc)[None, :]
    skip = np.concatenate([site_less, np.zeros((n, 1 + nc), bool)], axis=1)
    sc = np.where(X != 0.0, np.abs(X), np.concatenate([np.tile(TYPICAL, nc), np.ones(1 + nc)])[None, :])

    def L(Z):
        a, p, mu, v = oracle.mixn_derivatives(Z[:, : 8 * nc].reshape(n, nc, 8), Z[:, 8 * nc], Z[:, 8 * nc + 1 :], prec=1)
        return ga * a + gp * p + (gmu * mu).sum(axis=1) + (gv * v).sum(axis=1)

    fd, spread = np.zeros_like(X), np.zeros_like(X)
    for k in range(X.shape[1]):
        d, w2 = [], []
        for s in STEPS:
            h = np.where(skip[:, k], 0.0, s * sc[:, k])
            Xp, Xm = X.copy(), X.copy()
            Xp[:, k] += h
            Xm[:, k] -= h
            width = np.where(skip[:, k], 1.0, Xp[:, k] - Xm[:, k])  # the step actually taken
            d.append((L(Xp) - L(Xm)) / width)
            w2.append(width**2)
        fd[:, k] = np.where(skip[:, k], 0.0, (w2[0] * d[1] - w2[1] * d[0]) / np.where(skip[:, k], 1.0, w2[0] - w2[1]))
        spread[:, k] = np.abs(d[0] - d[1])
    return fd, spread, sc, skip


@pytest.mark.parametrize("nc", [1, 3, 6])
def test_exact_gradient_vs_richardson_differences(oracle, nc):
    """Every seeded column (zero-valued kappa_ab / epsilon_k_ab / mu and the site counts of the associating component
    included; only na, nb of site-less components cannot be differenced, see _richardson) against Richardson-extrapolated
    central differences of the long-double forward evaluation, 100 rows.

    Measure: the log-derivative, |x_k| |g_k - fd_k| / max_j |x_j g_j| per row (relative steps make the differences' error
    uniform in x dL/dx; x = the step scale).  Bar = what the differences can deliver, per entry:
      * rounding: the forward outputs are rounded to double (u = 1.1e-16) and L is summed in double, |dL| <= 4 u Tsum with
        Tsum = |ga a| + |gp p| + sum |gmu mu| + sum |gv v|; two evaluations per difference over a width 2 s x, weights 4/3
        and 1/3 at steps s1/2 and s1: <= 12 u Tsum / (s1 x), i.e. 1.3e-10 Tsum / max|x g| in the measure (Tsum / max|x g| is
        10 ... 100 on gas rows, whose gv . v terms of size 1e-3 / rho cancel);
      * truncation: |d(h1) - d(h2)|, the whole h^2 term that the extrapolation removes (near a mechanical spinodal, |v| >> 1 /
        rho, the fifth derivative is large: 4e-7 at one row of nc = 6, 4e-11 with ten times smaller steps).
    Conditions, so that the per-entry bar hides nothing: nine rows in ten have every bar below 1e-8 (the rest are the gas rows
    with the strongest cancellation and the near-spinodal rows), and the median row agrees to 1e-9 whatever its bar.
    Measured, nc = 1 / 3 / 6: largest error 3.8e-11 / 1.0e-9 / 4.3e-7, median over the rows 1.4e-11 / 3.5e-11 / 5.0e-11;
    largest error / bar 0.39 / 0.45 / 0.41; row bar, median 5.5e-10 / 1.2e-9 / 9.5e-10, 0.9 quantile 4.8e-9 / 8.0e-9 / 6.4e-9;
    rows with a bar above 1e-8: 0 / 9 / 10 of 100."""
    n = 100
    P, T, rho = random_rows(n, nc, 700 + nc)
    w = _weights(n, nc, 750 + nc)
    g = oracle.mixn_derivatives_vjp_exact(P, T, rho, *w, prec=1)
    assert g.shape == (n, 9 * nc + 1) and np.isfinite(g).all()
    fd, spread, sc, skip = _richardson(oracle, P, T, rho, w)
    a, p, mu, v = oracle.mixn_derivatives(P, T, rho, prec=1)
    tsum = np.abs(w[0] * a) + np.abs(w[1] * p) + np.abs(w[2] * mu).sum(axis=1) + np.abs(w[3] * v).sum(axis=1)
    lg = np.where(skip, 0.0, np.abs(sc * g)).max(axis=1, keepdims=True)
    err = np.where(skip, 0.0, sc * np.abs(g - fd)) / lg
    bar = 12 * 1.1e-16 / STEPS[0] * tsum[:, None] / lg + sc * spread / lg
    loose = (np.where(skip, 0.0, bar) > 1e-8).any(axis=1)
    print(f"nc={nc}: max err {err.max():.2e} median row {np.median(err.max(axis=1)):.2e} max err/bar "
          f"{np.where(skip, 0.0, err / bar).max():.2f} rows with a bar > 1e-8: {loose.sum()}")
    row_bar = np.where(skip, 0.0, bar).max(axis=1)
    print(f"row bar, quantiles 0.5 / 0.9 / 1: {np.quantile(row_bar, [0.5, 0.9, 1.0])}")
    assert np.quantile(row_bar, 0.9) < 1e-8  # the bars hide nothing: nine rows in ten are held below 1e-8 in every column
    assert np.median(err.max(axis=1)) < 1e-9  # and, bars aside, the typical row agrees to the rounding estimate at Tsum = 8 max|x g|
    assert (err <= bar).all(), (err / bar).max()
    # where nothing is differenced the gradient is still the formula's: 0 on rows without sites
    no_sites = (P[:, :, 6] + P[:, :, 7]).sum(axis=1) == 0.0
    assert np.all(g[no_sites][:, [8 * c + q for c in range(nc) for q in (4, 5, 6, 7)]] == 0.0)
    assert np.all(g[:, :8 * nc].reshape(n, nc, 8)[:, :, 3][P[:, :, 3] == 0.0] == 0.0)  # mu = 0: exactly 0


@pytest.mark.parametrize("nc", [1, 3, 6])
def test_exact_gradient_of_a_is_mu(oracle, nc):
    """L = a: dL/drho_i = mu_i, the tangent of DualN against the eps1 part of the HyperDual, both in long double and rounded
    to double once.  The two are not the same number: the forward evaluation keeps the parameters as doubles and forms their
    combinations (sqrt(eps_i eps_j), sigma_ij^3 m_i m_j, mu^2 / (m sigma^3 eps)) in double, the gradient carries them in long
    double.  Bar 2e-14 max(1, |mu_i|): u = 1.1e-16 on each of about six such combinations, whose log-sensitivities |d mu / d ln
    x| reach 30 max(1, |mu|) in the liquid rows.  Measured 2.2e-15 / 2.9e-15 / 2.1e-15 (nc = 2 against the binary code, which
    is long double in the parameters too: 0)."""
    n = 100
    P, T, rho = random_rows(n, nc, 700 + nc)
    z = np.zeros((n, nc))
    g = oracle.mixn_derivatives_vjp_exact(P, T, rho, np.ones(n), np.zeros(n), z, z, prec=1)
    _, _, mu, _ = oracle.mixn_derivatives(P, T, rho, prec=1)
    d = np.abs(g[:, 8 * nc + 1 :] - mu) / np.maximum(1.0, np.abs(mu))
    print(f"nc={nc}: max |da/drho - mu| / max(1, |mu|) = {d.max():.2e}")
    assert d.max() < 2e-14


def test_exact_gradient_nc2_equals_the_binary_long_double_code(oracle):
    """nc = 2, k_ij = 0: the binary model (oracle/pcsaft_mix.hpp, written separately from pcsaft_mixn.hpp and generic in every
    parameter) has two long-double functions to compare with, and no more:
      * mix_derivatives_exact: values only, so mu_i = d a / d rho_i checks the rho columns of L = a;
      * mix_bubble_dew_grad(exact=True): the gradient of the bubble / dew pressure formula (pcsaft_mix.py:459-468) at FIXED
        densities with respect to the 16 parameters and T.  The formula is p = -(a_i + p_s v + g - 1) / (1 / rho_i - v) T
        P_UNIT with v = y . v_s, g = y . (log(rho_inc / rho_spec) - mu_s), a_i = a(rho_inc) / rho_i: a function of (a, p, mu,
        v) at the specified phase and of a at the incipient one, so its gradient is the sum of two VJPs with the upstream
        weights written out below, plus p / T in the T column.  This checks all 16 parameter columns and the T column.
    No binary function differentiates p, mu or v with respect to the densities; those columns are covered by the differences
    above only.  Rows: 100 random binary states as the specified phase, the same rows at another seed's densities as the
    incipient one (no equilibrium needed: the formula is differentiated wherever it is evaluated).
    Bars: mu 1e-15 max(1, |mu|) (both sides long double in everything, rounded once; measured 0).  The formula's gradient,
    relative to the row's largest component: the upstream weights are formed here in double from outputs rounded to double,
    and the numerator a_i + p_s v + g - 1 and the denominator 1 / rho_i - v cancel, so the bar is 50 u cond per row, cond =
    sum |terms| / |numerator| + 2 (1 / rho_i + |v|) / |denominator| (the denominator enters squared); 50 = about ten rounded
    operations behind each weight times the five weighted pieces that are then summed.  Its median must stay below 1e-13.
    Measured: largest error 1.1e-12 at 0.74 of its bar; bar median 2.5e-14, largest 1.5e-12."""
    n, nc = 100, 2
    P, T, rho = random_rows(n, nc, 702)
    _, _, rho_inc = random_rows(n, nc, 703)
    kij = np.zeros((n, 2))
    _, _, mu2, _ = oracle.mix_derivatives_exact(P, kij, T, rho)
    z = np.zeros((n, nc))
    g = oracle.mixn_derivatives_vjp_exact(P, T, rho, np.ones(n), np.zeros(n), z, z, prec=1)
    d = np.abs(g[:, 17:] - mu2) / np.maximum(1.0, np.abs(mu2))
    print(f"mu: {d.max():.2e}")
    assert d.max() < 1e-15
    # the dew formula: specified phase = vapour slot rho4[:, :2], incipient = liquid slot
    val, gb = oracle.mix_bubble_dew_grad(P, kij, T, np.concatenate([rho, rho_inc], axis=1), dew=True, exact=True)
    a_s, p_s, mu_s, v_s = oracle.mix_derivatives_exact(P, kij, T, rho)
    a_inc = oracle.mix_derivatives_exact(P, kij, T, rho_inc)[0]
    rho_i = rho_inc.sum(axis=1)
    y = rho_inc / rho_i[:, None]
    v = (y * v_s).sum(axis=1)
    num = a_inc / rho_i + p_s * v + (y * (np.log(rho_inc / rho) - mu_s)).sum(axis=1) - 1.0
    den = 1.0 / rho_i - v
    c = T * (1.380649e-23 / 1e-30)
    assert np.max(np.abs(-num / den * c / val - 1.0)) < 1e-12
    g_spec = oracle.mixn_derivatives_vjp_exact(P, T, rho, z[:, 0], -v / den * c, y * (c / den)[:, None],
                                               y * ((-p_s / den - num / den**2) * c)[:, None], prec=1)
    g_inc = oracle.mixn_derivatives_vjp_exact(P, T, rho_inc, -c / (rho_i * den), z[:, 0], z, z, prec=1)
    mine = (g_spec + g_inc)[:, :17]
    mine[:, 16] += val / T
    want = np.concatenate([gb[:, :16], gb[:, 18:19]], axis=1)
    e = np.abs(mine - want).max(axis=1) / np.abs(want).max(axis=1)
    # the composition above is done in double on outputs rounded to double: its numerator and denominator cancel
    parts = np.abs(a_inc / rho_i) + np.abs(p_s * v) + np.abs(y * np.log(rho_inc / rho)).sum(axis=1) + np.abs(y * mu_s).sum(axis=1) + 1.0
    cond = parts / np.abs(num) + 2.0 * (1.0 / rho_i + np.abs(v)) / np.abs(den)
    bar = 50 * 1.1e-16 * cond
    print(f"bubble/dew formula gradient: {e.max():.2e}, err / bar {np.max(e / bar):.2f}, bar median {np.median(bar):.1e} max {bar.max():.1e}")
    assert np.median(bar) < 1e-13 and (e <= bar).all()
