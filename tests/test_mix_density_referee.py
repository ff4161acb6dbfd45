"""CPU: the referee and the input set of tests/test_mix_density_gpu.py, on their own (tests/tools/mix_density_referee.py).

  1. At most CAP of the rows of any (class, temperature factor, pressure) cell of a phase are dropped.
  2. At the factor-1 pressures -- the oracle's own bubble / dew pressure -- the referee's liquid / vapour density is the sum of
     the specified phase's partial densities of that bubble / dew solution (rho4) to 1e-12: the referee is tied to a quantity
     the bubble / dew tests already pin.
  3. The referee's gradient is the derivative of the referee's root: central differences of the whole solve in T, p and x.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import mix_density_referee as ref  # noqa: E402

PHASES = (ref.LIQUID, ref.VAPOUR)


@pytest.mark.parametrize("phase", PHASES)
def test_dropped_rows_stay_below_the_cap(oracle, phase):
    c = ref.inputs(oracle, phase)
    print("phase %d: %d rows, %d compared, %d kept; referee status counts %s; largest dropped share of a cell %.3f" % (
        phase, c.n, c.compared.sum(), c.keep.sum(), np.bincount(c.status, minlength=4), c.dropped_share.max()))
    assert len(c.dropped_share) == c.nblocks * 3 * 6
    assert (c.dropped_share <= ref.CAP).all(), c.dropped_share
    assert np.isfinite(c.grad[c.keep]).all() and np.isfinite(c.grad64[c.keep]).all()
    assert (c.dpdrho[c.keep] >= ref.MIN_SLOPE).all()


@pytest.mark.parametrize("phase", PHASES)
def test_factor_one_density_is_the_bubble_dew_solution(oracle, phase):
    c = ref.inputs(oracle, phase)
    rows = c.keep & (c.block == 0)
    spec = (c.base_rho4[:, 0:2] if phase == ref.VAPOUR else c.base_rho4[:, 2:4]).sum(axis=1)
    err = np.abs(c.rho[rows] / spec[rows] - 1.0)
    print("phase %d: %d rows, largest |rho_referee / rho_bubble_dew - 1| = %.2e" % (phase, rows.sum(), err.max()))
    assert rows.sum() >= 500
    assert err.max() <= 1e-12


@pytest.mark.parametrize("phase", PHASES)
def test_gradient_is_the_derivative_of_the_root(oracle, phase):
    """d rho / d(T, p, x) of the referee against central differences of the referee's own solve on four rows per class, as
    logarithmic derivatives d ln rho / d ln(T, p, x) (of order 1, but 1e-3 ... 1e-8 for a liquid's pressure: a relative
    measure of that column would only see the differences' rounding).  Bar 1e-8: step 1e-5 relative, truncation 1e-10 x the
    third logarithmic derivative, rounding 1e-16 / 1e-5."""
    c = ref.inputs(oracle, phase)
    rows = np.concatenate([np.nonzero(c.keep & (c.cls == k) & (c.block == 1) & (c.x > 0.01) & (c.x < 0.99))[0][:4] for k in range(6)])
    assert len(rows) == 24
    P, K, T, p, x = c.P[rows], c.K[rows], c.T[rows], c.p[rows], c.x[rows]
    for col, name in ((18, "T"), (19, "p"), (20, "x")):
        h = 1e-5
        args = lambda s: (T * (1 + s * h) if col == 18 else T, p * (1 + s * h) if col == 19 else p, x * (1 + s * h) if col == 20 else x)
        up, _, su = ref.solve(oracle, P, K, *args(+1), phase)
        dn, _, sd = ref.solve(oracle, P, K, *args(-1), phase)
        assert (su == ref.OK).all() and (sd == ref.OK).all()
        base = (T, p, x)[col - 18]
        fd = (up - dn) / (2 * h * base)
        err = np.abs(fd - c.grad[rows, col]) * base / c.rho[rows]
        print("phase %d d ln rho / d ln %s: largest difference to central differences %.2e (largest value %.2e)" % (
            phase, name, err.max(), np.abs(c.grad[rows, col] * base / c.rho[rows]).max()))
        assert err.max() <= 1e-8
