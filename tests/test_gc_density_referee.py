"""CPU: the referee and the input set of tests/test_gc_density_gpu.py, on their own (tests/tools/gc_density_referee.py).

  1. At most CAP of the rows of any (class, temperature factor, pressure block) cell of a phase are dropped, and every class
     of the base set has kept rows in every block.
  2. The referee's roots reproduce p_spec: |p(rho) - p_spec| <= 1e-13 max(p_spec, s rho) with p the oracle's long-double
     pressure at the root and s = dp/drho there.  The root is stored as a double, so its last bit alone moves p by
     1.1e-16 s rho; relative to p_spec itself no stored liquid root can be held (p_spec / (s rho) goes down to 1e-9 on these
     rows).  The figure relative to max(p_spec, rho) is printed next to it.
  3. At the factor-1 pressures -- the oracle's own bubble / dew pressure -- the referee's liquid / vapour density is the sum of
     the specified phase's partial densities of that bubble / dew solution (rho4) to 1e-10.

Measured (both phases): no row dropped (liquid 5760 of 5760 kept, vapour 3456 of 3456); see the printed figures.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import gc_density_referee as ref  # noqa: E402

PHASES = (ref.LIQUID, ref.VAPOUR)


@pytest.mark.parametrize("phase", PHASES)
def test_dropped_rows_stay_below_the_cap(oracle, phase):
    c = ref.inputs(oracle, phase)
    worst = max(c.dropped_share.values())
    print("phase %d: %d rows, %d compared, %d kept; referee status counts %s; largest dropped share of a cell %.3f" % (
        phase, c.n, c.compared.sum(), c.keep.sum(), np.bincount(c.status, minlength=4), worst))
    assert len(c.dropped_share) == c.nblocks * 3 * len(c.classes)
    assert worst <= ref.CAP, c.dropped_share
    for blk in range(c.nblocks):
        for k in c.classes:
            assert (c.keep & (c.block == blk) & (c.cls == k)).any(), (blk, k)
    assert np.isfinite(c.grad_row[c.keep]).all() and np.isfinite(c.rho[c.keep]).all()
    assert (c.dpdrho[c.keep] >= ref.MIN_SLOPE).all()
    if phase == ref.LIQUID:  # the pure-limit blocks are served: the oracle is finite at an exactly zero partial density
        ends = c.keep & ((c.x == 0.0) | (c.x == 1.0))
        assert ends.sum() >= 0.9 * 2 * c.base.n


@pytest.mark.parametrize("phase", PHASES)
def test_roots_reproduce_the_pressure(oracle, phase):
    c = ref.inputs(oracle, phase)
    k = np.nonzero(c.keep)[0]
    p = ref.pressure(c.m, c.row[k], c.T[k], c.x[k], c.rho[k])
    ps = c.p[k] * ref.P_RED / c.T[k]
    err = np.abs(p - ps) / np.maximum(ps, c.dpdrho[k] * c.rho[k])
    plain = np.abs(p - ps) / np.maximum(ps, c.rho[k])
    print("phase %d: %d roots, largest |p(rho) - p_spec| / max(p_spec, s rho) = %.2e (bar 1e-13), / max(p_spec, rho) = %.2e" % (
        phase, len(k), err.max(), plain.max()))
    assert err.max() <= 1e-13


@pytest.mark.parametrize("phase", PHASES)
def test_factor_one_density_is_the_bubble_dew_solution(oracle, phase):
    c = ref.inputs(oracle, phase)
    rows = c.keep & (c.block == 0)
    spec = (c.base_rho4[:, 0:2] if phase == ref.VAPOUR else c.base_rho4[:, 2:4]).sum(axis=1)
    err = np.abs(c.rho[rows] / spec[rows] - 1.0)
    print("phase %d: %d rows, largest |rho_referee / rho_bubble_dew - 1| = %.2e (bar 1e-10)" % (phase, rows.sum(), err.max()))
    assert rows.sum() >= 0.9 * c.base.n
    assert err.max() <= 1e-10
