"""CPU: the referee of the gc incipient-composition gradient (tests/tools/gc_incipient_referee.py) measured by the oracle alone.

The Richardson machinery that produces the y blocks is applied to p as well, where the oracle has an exact answer
(gc_bubble_dew_vjp_exact: grad_row, grad_kab, grad_seg): e = the error of those p blocks per group of gc_point_rows.groups, in
the measures of gc_point_rows (row_error, kab_error, seg_error).  The GPU test's bars for the y blocks are max(10 e, 1e-8).

Measured (H = 3e-6, 720 rows per problem): see the figures in test_referee_error_and_dropped_share's docstring.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import gc_incipient_referee as ref  # noqa: E402
import gc_point_rows as gp  # noqa: E402

name = lambda dew: "dew" if dew else "bubble"


@pytest.mark.parametrize("dew", (False, True))
def test_referee_error_and_dropped_share(oracle, dew):
    """Measured, H = 3e-6 (largest over the groups; the bars are 10 e or the floor 1e-8):
      bubble: 720 of 720 rows kept; e phi 6.7e-11, T 5.6e-11, k_ab 2.0e-9 (bar 2.0e-8), table 2.9e-10;
              h^2 estimates of the kept rows <= 3.4e-9; y in [8.2e-13, 1 - 3.7e-12]
      dew:    717 of 720 rows kept (largest dropped share of a class 1.6 %); e phi 7.3e-11, T 5.7e-11, k_ab 2.3e-9
              (bar 2.3e-8), table 2.9e-10; h^2 estimates <= 5.3e-9; y in [7.8e-14, 1 - 4.8e-14]"""
    c = ref.referee(oracle, dew)
    r = c.rows
    print("\n%-6s H = %.0e: kept %d of %d, largest dropped share of a class %.4f; est phi %.2e T %.2e tab %.2e on the kept rows" % (
        name(dew), ref.H, c.keep.sum(), r["m"], max(c.dropped_share.values()), c.est["phi"][c.keep].max(),
        c.est["T"][c.keep].max(), c.est["tab"][c.keep].max()))
    assert max(c.dropped_share.values()) <= ref.CAP, c.dropped_share
    assert set(c.dropped_share) == {0, 1, 2, 3, 5, 6}, "every model class of the set"
    for gname, g in c.groups.items():
        e_seg = g.e_seg[~np.isnan(g.e_seg)]
        print("   %-15s e: phi %.2e T %.2e k_ab %.2e table %.2e -> bars %.2e %.2e %.2e %.2e" % (
            gname, g.e_row["phi"], g.e_row["T"], g.e_kab, e_seg.max(), g.bar_row["phi"], g.bar_row["T"], g.bar_kab, g.bar_seg.max()))
        assert np.isfinite([g.e_row["phi"], g.e_row["T"], g.e_kab]).all() and np.isfinite(e_seg).all() and len(e_seg) >= 3
        for bar in (g.bar_row["phi"], g.bar_row["T"], g.bar_kab, g.bar_seg.max()):
            assert bar < 1e-6, "a referee this loose pins nothing"
        assert (g.w[~c.keep] == 0.0).all()
        assert np.isfinite(g.kab_y).all() and np.isfinite(g.seg_y).all()
    k = c.keep
    y_small = np.minimum(c.y, 1.0 - c.y)
    print("   y in [%.2e, 1 - %.2e]; rows whose y rounds to 1.0 as a double: %d" % (c.y[k].min(), (1.0 - c.y[k]).min(), (c.y[k] == 1.0).sum()))
    assert ((c.y[k] > 0) & (c.y[k] <= 1)).all() and y_small[k].min() < 1e-9, "trace rows are in the set"
    assert np.isfinite(c.d["row"].Ry[k]).all() and np.isfinite(c.d["seg"].Ry[k]).all() and np.isfinite(c.d["kab"].Ry[k]).all()
    # '>C<' has epsilon_k = 0: that entry is not a direction
    ident = r["enc"]["ident"]
    assert not c.d["reported"][ident.index(">C<"), 2] and c.d["reported"][ident.index(">C<"), 0]


def test_quotient_is_the_derivative_along_constant_pressure():
    """dy|_p = J_y - J_y[T] J_p / J_p[T]: a made-up linear pair p = a . theta + b T, y = c . theta + d T"""
    rng = np.random.default_rng(0)
    Jp, Jy = rng.normal(size=(4, 7)), rng.normal(size=(4, 7))
    q = ref.quotient(Jp, Jy)
    dtheta = rng.normal(size=(4, 6))
    dp = rng.normal(size=4)
    dT = (dp - (Jp[:, :6] * dtheta).sum(axis=1)) / Jp[:, 6]
    dy = (Jy[:, :6] * dtheta).sum(axis=1) + Jy[:, 6] * dT
    assert np.allclose(dy, (q[:, :6] * dtheta).sum(axis=1) + q[:, 6] * dp, rtol=1e-12, atol=1e-12)
