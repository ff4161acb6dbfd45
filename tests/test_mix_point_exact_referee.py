"""CPU: the exact referee of the binary bubble / dew gradient blocks (tests/tools/mix_point_exact.py) measured by the oracle alone.

  1. Two exact routes to the pressure block agree: the implicit-function assembly over oracle.mix_derivatives_vjp_exact and
     oracle.mix_bubble_dew_grad(exact=True) (the gradient of the reference's final Newton step), every kept row, all 19 columns,
     within 1e-12 of the row's largest component.
  2. The composition block agrees with the Richardson referee (tests/tools/mix_incipient_referee.py) on its kept rows and in its
     checked directions within that referee's own bar: the independent anchor.
  3. The caps that keep tests/test_mix_point_exact_gpu.py from hiding a failure behind a bar of 10 e_row: at most 8 of the 32 rows
     of a (class, factor, problem) cell and at most 3 % of the kept rows are not tight, every class keeps 16 tight rows, every
     zero-parameter column that the exact y block fills is exercised by 8 rows.

Measured (every run prints them).  Routes: 1.3e-13 (bubble; 3.1e-15 without the one row whose vapour holds 5e-26 A^-3 of a
component) / 2.4e-14 (dew).  Against Richardson: 1.59e-8 / 5.72e-9 -- the figures so far reported as the kernel's error are that
referee's own; 3063 of 10754 / 3130 of 10830 entries are directions it skips.  e_row of the twin: median 5e-15 ... 1.3e-14,
90th percentile at most 7.7e-14; rows not tight, p / y: bubble 7 / 3, dew 9 / 12, all of class 2, at most 7 of a cell and 2.1 %
of the kept rows; the worst row reaches 1.2e-5.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import mix_incipient_referee as ric  # noqa: E402
import mix_point_exact as ex  # noqa: E402
import mix_temperature_referee as tref  # noqa: E402

name = lambda dew: "dew" if dew else "bubble"
PROBLEMS = (False, True)


@pytest.mark.parametrize("dew", PROBLEMS)
def test_two_exact_routes_agree_on_the_pressure_block(oracle, dew):
    """Measured: bubble 1.3e-13, dew 2.4e-14 (566 / 576 kept rows)."""
    c = ex.inputs(oracle, dew)
    k = c.keep
    assert np.isfinite(c.Jp[k]).all() and np.isfinite(c.Jy[k]).all() and np.isfinite(c.Jp64[k]).all() and np.isfinite(c.Jy64[k]).all()
    err = ex.row_error(c.Jp, c.grad)
    print("%-6s p block, assembly vs mix_bubble_dew_grad(exact=True): max %.2e, median %.2e on %d rows, 19 columns" % (
        name(dew), err[k].max(), np.median(err[k]), k.sum()))
    assert (err[k] <= 1e-12).all(), (np.nonzero(k & ~(err <= 1e-12))[0], err[k].max())
    # the zero-parameter convention is the same in both routes: the same entries are exactly zero
    assert np.array_equal(c.Jp[k] == 0.0, c.grad[k] == 0.0)


@pytest.mark.parametrize("dew", PROBLEMS)
def test_composition_block_against_the_richardson_referee(oracle, dew):
    """Measured: bubble 1.6e-8 (bar 2.5e-7), dew 5.7e-9 (bar 9.5e-8): the Richardson referee's own error."""
    c = ex.inputs(oracle, dew)
    r = ric.inputs(oracle, dew)
    k = r.keep_y
    assert not (k & ~c.keep).any()
    err = ric.row_error(c.Jy, r.Ry, r.checked)
    unchecked = int((~r.checked[k]).sum())
    print("%-6s y block, exact vs Richardson: max %.2e, median %.2e on %d rows (bar %.2e); %d of %d entries not checked by it" % (
        name(dew), err[k].max(), np.median(err[k]), k.sum(), r.bar, unchecked, k.sum() * ex.N_DIRS))
    assert (err[k] <= r.bar).all(), (np.nonzero(k & ~(err <= r.bar))[0], err[k].max())
    lead = np.abs(c.Jy[k]).argmax(axis=1)
    print("%-6s rows whose largest exact dy/dtheta is a direction Richardson skips: %d" % (
        name(dew), int((~r.checked[k][np.arange(k.sum()), lead]).sum())))


@pytest.mark.parametrize("dew", PROBLEMS)
def test_caps_on_the_bars(oracle, dew):
    """Measured (block p / y): rows not tight bubble 7 / 3, dew 9 / 12; see the printed lines."""
    c = ex.inputs(oracle, dew)
    k = c.keep
    for s in "py":
        e, tight = getattr(c, "e_" + s), getattr(c, "tight_" + s)
        loose = k & ~tight
        worst_cell = max(int(loose[c.cell == j].sum()) for j in np.unique(c.cell))
        per_class = [int((tight & (c.cls == j)).sum()) for j in range(tref.N_CLASSES)]
        print("%-6s %s block: e_row median %.1e, p90 %.1e, max %.1e; not tight %d of %d (%.2f %%), classes %s, worst cell %d / 32; "
              "tight rows per class %s" % (name(dew), s, np.median(e[k]), np.quantile(e[k], 0.9), e[k].max(), loose.sum(), k.sum(),
                                           100.0 * loose.sum() / k.sum(), sorted(set(c.cls[loose].tolist())), worst_cell, per_class))
        assert np.isfinite(e[k]).all()
        assert worst_cell <= 8
        assert loose.sum() <= 0.03 * k.sum()
        assert min(per_class) >= 16
    filled = np.nonzero(c.zero_entry_y.any(axis=0))[0]
    counts = {ex.COLUMNS[j]: int((c.zero_entry_y[:, j] & c.tight_y).sum()) for j in filled}
    print("%-6s zero-parameter columns the exact y block fills, tight rows each: %s" % (name(dew), counts))
    assert len(filled) > 0 and min(counts.values()) >= 8, counts
    lead = np.abs(c.Jy[k]).argmax(axis=1)
    print("%-6s zero-parameter entries: %d of %d are non-zero in the exact y block, the row's largest component in %d rows" % (
        name(dew), int(c.zero_entry_y.sum()), int((c.zero_param & k[:, None]).sum()),
        int(c.zero_entry_y[k][np.arange(k.sum()), lead].sum())))
    # (classes 2 and 5 put the sites on either component: no row of theirs has every column of the class non-zero)
    print("%-6s rows with every column of their class non-zero, per class: %s; zero-parameter columns per class: %s" % (
        name(dew), [int(c.full_rows[j].sum()) for j in range(tref.N_CLASSES)], [len(c.zero_rows[j]) for j in range(tref.N_CLASSES)]))
    assert all(c.full_rows[j].sum() >= 16 for j in (0, 1, 3, 4))


def test_solve3_and_row_error():
    """the 3 x 3 elimination against numpy's on random systems, one of them needing both row exchanges"""
    rng = np.random.default_rng(1)
    J, B = rng.normal(size=(50, 3, 3)), rng.normal(size=(50, 3, 4))
    J[0] = [[1e-9, 1.0, 2.0], [1.0, 1e-9, 3.0], [4.0, 5.0, 6.0]]
    for dt, tol in ((np.float64, 1e-10), (np.longdouble, 1e-10)):
        x = ex.solve3(J.astype(dt), B.astype(dt)).astype(np.float64)
        assert np.allclose(x, np.linalg.solve(J, B), rtol=tol, atol=tol)
