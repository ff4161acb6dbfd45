"""CPU: the referee behind tests/test_mix_temperature_gpu.py (tests/tools/mix_temperature_referee.py) stands on its own.

  1. the cap: at most 10 % of the rows of any (class, factor, problem) cell of the input set are dropped in advance;
  2. from both displaced starts (0.93 / 1.07 T_grid) the referee returns T_grid within 1e-12 relative, and the oracle's
     pressure at the returned T is p_spec within 1e-12;
  3. the referee gradient (implicit-function quotient of the oracle's exact pressure gradient) equals central differences of
     the WHOLE referee solve in k_ij and in p_spec on a few rows per class.  Bar 1e-5 relative: steps of 1e-4 (absolute in
     k_ij ~ 0.1, relative in p_spec) leave a truncation error of h^2 times a third-derivative ratio of order 10-100, i.e.
     <= 1e-6, and a rounding error of the solve (T to ~1e-13) over 2 h of ~1e-9.  dT/dk_ij is measured against
     max(|dT/dk_ij|, 1e-3 T): k_ij is dimensionless and a derivative far below T is a structural zero (a dew row at 117 K whose
     second component is a 1e-78 trace in the liquid has dT/dk_ij = 1e-41 K, and the differences return exactly 0).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import mix_temperature_referee as ref  # noqa: E402

PROBLEMS = (False, True)


@pytest.mark.parametrize("dew", PROBLEMS)
def test_cap_on_rows_dropped_in_advance(oracle, dew):
    c = ref.inputs(oracle, dew)
    print("dew" if dew else "bubble", "dropped per (factor, class) cell:", np.round(c.dropped_share, 3).reshape(len(ref.FACTORS), -1))
    assert c.n == len(ref.FACTORS) * ref.N_ROWS <= 576
    assert (c.dropped_share <= ref.CAP).all(), c.dropped_share


@pytest.mark.parametrize("dew", PROBLEMS)
def test_referee_returns_the_grid_temperature_from_displaced_starts(oracle, dew):
    c = ref.inputs(oracle, dew)
    k = c.keep
    for s in ref.STARTS[1:]:
        T, p, _ = ref.solve_temperature(oracle, c.P[k], c.K[k], c.z[k], c.p_spec[k], s * c.T[k], dew)
        assert np.isfinite(T).all(), (s, int((~np.isfinite(T)).sum()))
        eT, ep = np.abs(T / c.T[k] - 1.0), np.abs(p / c.p_spec[k] - 1.0)
        print("dew" if dew else "bubble", "start", s, "max |T/T_grid - 1| %.2e  max |p/p_spec - 1| %.2e" % (eT.max(), ep.max()))
        assert (eT <= 1e-12).all() and (ep <= 1e-12).all()


@pytest.mark.parametrize("dew", PROBLEMS)
def test_referee_gradient_equals_central_differences_of_the_solve(oracle, dew):
    c = ref.inputs(oracle, dew)
    rows = np.concatenate([np.nonzero(c.keep & (c.cls == k))[0][[0, 40, -1]] for k in range(ref.N_CLASSES)])
    P, K, z, ps, T0 = c.P[rows], c.K[rows], c.z[rows], c.p_spec[rows], c.T[rows]
    q = ref.gradient(oracle, P, K, T0, c.rho4[rows], dew)
    h = 1e-4
    solve = lambda K_, p_: ref.solve_temperature(oracle, P, K_, z, p_, T0, dew)[0]
    dK = np.zeros_like(K)
    dK[:, 0] = h
    fd_k = (solve(K + dK, ps) - solve(K - dK, ps)) / (2 * h)
    fd_p = (solve(K, ps * (1 + h)) - solve(K, ps * (1 - h))) / (2 * h * ps)
    ek = np.abs(fd_k - q[:, 16]) / np.maximum(np.abs(q[:, 16]), 1e-3 * T0)
    ep = np.abs(fd_p / q[:, 18] - 1.0)
    print("dew" if dew else "bubble", "dT/dk_ij: max rel %.2e   dT/dp: max rel %.2e" % (ek.max(), ep.max()))
    assert (q[:, 18] > 0).all()
    assert (ek <= 1e-5).all() and (ep <= 1e-5).all()
