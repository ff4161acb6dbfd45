"""CPU: the referee of the Henry's-law-constant tests (tests/tools/henry_referee.py) against judges it does not share code with.

* it keeps every row of the synthetic mixture batch, for either choice of the solute: finite ln H, finite 19-column gradient;
* its d rho_L / d(theta, T) -- the oracle's fixed-density gradient of the equilibrium-liquid-density formula, claimed to be the
  TOTAL derivative at the converged equilibrium -- agrees with central differences of the long-double VLE solve itself;
* with identical components and k_ij = 0 a trace of the "solute" is the solvent: H = rho_V k_B T exp(mu_res(rho_V)), the
  fugacity of the saturated vapour (equal fugacities of the two phases), from the pure-component oracle.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import henry_referee as hr  # noqa: E402

N = 720


def _batch():
    from feos_torch_amd.synthetic import mix_batch

    return mix_batch(N)[:3]


def test_the_referee_keeps_every_row(oracle):
    P, K, T = _batch()
    for solute in (0, 1):
        r = hr.reference(oracle, P, K, T, solute)
        assert not r["failed"].any(), np.nonzero(r["failed"])[0]
        assert np.isfinite(r["lnh"]).all() and np.isfinite(r["grad"]).all()
        assert np.isfinite(r["d_lnh"]).all() and np.isfinite(r["d_grad"]).all()  # the twin solves every row as well
        print("solute %d: ln H [Pa] in [%.2f, %.2f]; twin - referee: ln H max %.2e (median %.1e), gradient max %.2e of the row's "
              "largest component (median %.1e); rows above 1e-11: %d / %d" % (solute, r["lnh"].min(), r["lnh"].max(), r["d_lnh"].max(),
                                                                             np.median(r["d_lnh"]), r["d_grad"].max(), np.median(r["d_grad"]),
                                                                             (r["d_lnh"] > 1e-11).sum(), (r["d_grad"] > 1e-11).sum()))


def test_density_derivative_is_the_total_derivative(oracle):
    """Central differences of rho_L from pure_vle(prec=1) at relative step h: truncation ~h^2 |rho'''| rho^2, rounding of the
    returned doubles ~1e-16 / h.  h = 1e-5 leaves ~1e-10 + 1e-11 relative to the row's largest component times a modest
    third-derivative factor (taken as 10): asserted at 1e-9, the measured figure is printed."""
    P, _, T = _batch()
    n = 120
    par, T = np.ascontiguousarray(P[:n, 0, :]), np.ascontiguousarray(T[:n])
    rv, rl, st, _, _ = oracle.pure_vle(par, T, prec=1)
    assert not st.any()
    exact = hr.drho_l(oracle, par, T, rv, rl, prec=1)
    X = np.concatenate([par, T[:, None]], axis=1)
    h_rel = 1e-5
    cd = np.zeros((n, 9))
    for k in range(9):
        h = h_rel * np.abs(X[:, k])
        if not h.any():
            continue
        v = []
        for f in (-2.0, -1.0, 1.0, 2.0):
            Y = X.copy()
            Y[:, k] += f * h
            _, l, s, _, _ = oracle.pure_vle(np.ascontiguousarray(Y[:, :8]), np.ascontiguousarray(Y[:, 8]), prec=1)
            assert not s.any()
            v.append(l)
        with np.errstate(invalid="ignore", divide="ignore"):
            cd[:, k] = np.where(h > 0, (v[0] - 8.0 * v[1] + 8.0 * v[2] - v[3]) / (12.0 * h), 0.0)
    # zero-valued parameters: the central difference does not move them (the row keeps its class); compare where it does.
    # Scale: the logarithmic derivatives x d rho_L / dx of the row
    moved = X != 0.0
    scale = np.abs(exact * X).max(axis=1)[:, None]
    err = np.where(moved, np.abs(exact - cd) * np.abs(X) / scale, 0.0)
    print("d rho_L / d(theta, T): max |referee - central difference| = %.2e of the row's largest logarithmic derivative" % err.max())
    assert err.max() <= 1e-9


def test_identical_components_give_the_solvents_own_fugacity(oracle):
    P, _, T = _batch()
    Q = P.copy()
    Q[:, 1, :] = Q[:, 0, :]
    # identical self-associating components cross-associate by the mean combining rule: exactly the pure fluid
    K = np.zeros((N, 2))
    for solute in (0, 1):
        v = hr.value(oracle, Q, K, T, solute, prec=1)
        assert not v["failed"].any()
        par = np.ascontiguousarray(Q[:, 0, :])
        rho_v = v["rho_v"]
        mu_v = oracle.mix_derivatives_exact(Q, K, T, np.stack([rho_v, np.zeros(N)], axis=1))[2][:, 0]
        ln_f = np.log(rho_v * T * hr.KT_A3) + mu_v
        # the same chemical potential from the pure-component oracle: mu = a' = (p - rho + a) / rho
        a, p, _ = oracle.pure_derivatives(par, T, rho_v, prec=1)
        mu_pure = (p - rho_v + a) / rho_v
        err_model = np.abs(mu_v - mu_pure)
        err = np.abs(v["lnh"] - ln_f)
        print("solute %d: max |ln H - ln f_V| = %.2e; mixture vs pure oracle mu at rho_V: %.2e" % (solute, err.max(), err_model.max()))
        assert err.max() <= 1e-12  # absolute in ln H = relative in H
        assert err_model.max() <= 1e-12
