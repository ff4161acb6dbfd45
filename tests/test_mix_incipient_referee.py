"""CPU: the referee of the incipient-composition gradient (tests/tools/mix_incipient_referee.py) measured by the oracle alone.

The Richardson machinery that produces the y block is applied to p as well, where the oracle has an exact answer
(mix_bubble_dew_grad(exact=True)): e = the largest error of that p block on the kept rows, relative to the row's largest
component.  The GPU test's bar for jac_y is max(10 e, 1e-8): 1e-8 is what tests/test_dilute_gpu.py applies to
pcs_mix_jacobian, the factor 10 covers the difference in conditioning between p and y.

Measured (H = 3e-6): bubble e = 2.5e-8 (bar 2.5e-7), 566 of 576 rows kept, largest dropped share of a cell 3/32;
dew e = 9.5e-9 (bar 9.5e-8), 570 of 576 kept, largest dropped share 3/32.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import mix_incipient_referee as ref  # noqa: E402

name = lambda dew: "dew" if dew else "bubble"


@pytest.mark.parametrize("dew", (False, True))
def test_referee_error_and_dropped_share(oracle, dew):
    c = ref.inputs(oracle, dew)
    k = c.keep_y
    print("%-6s H = %.0e: kept %d of %d (set keeps %d), largest dropped share of a cell %.4f" % (
        name(dew), ref.H, k.sum(), c.n, c.keep.sum(), c.dropped_share_y.max()))
    print("%-6s e = %.2e (Richardson p block vs exact, kept rows) -> bar = %.2e; est_y <= %.2e, est_p <= %.2e on the kept rows" % (
        name(dew), c.e, c.bar, c.est_y[k].max(), c.est_p[k].max()))
    assert (c.dropped_share_y <= ref.CAP).all(), c.dropped_share_y
    assert np.isfinite(c.e) and c.bar == max(10.0 * c.e, 1e-8)
    assert c.bar < 1e-6, "a referee this loose pins nothing"
    # every kept row: all displaced solves sound, both blocks finite on the checked directions, 0 < y < 1
    assert not c.fd_bad[k].any() and (c.est_y[k] <= ref.BAR_FLOOR).all()
    assert np.isfinite(c.Ry[k][c.checked[k]]).all() and np.isfinite(c.Rp[k][c.checked[k]]).all()
    # (a trace component below 1.1e-16 leaves y = 1.0 as a double: such rows stay in the set, their gradient is differenced
    # through the trace component's own mole fraction)
    print("%-6s rows whose y rounds to 1.0 as a double: %d" % (name(dew), (c.y[k] == 1.0).sum()))
    assert ((c.y[k] > 0) & (c.y[k] <= 1)).all()
    assert set(np.unique(c.cls[k])) == set(range(6)), "every association class of the set"
    # m, sigma, epsilon of both components, kij0 and T are displaced on every row
    assert c.checked[k][:, [0, 1, 2, 8, 9, 10, 18]].all()


def test_quotient_is_the_derivative_along_constant_pressure():
    """dy|_p = J_y - J_y[T] J_p / J_p[T]: a made-up linear pair p = a . theta + b T, y = c . theta + d T"""
    rng = np.random.default_rng(0)
    Jp, Jy = rng.normal(size=(4, 19)), rng.normal(size=(4, 19))
    q = ref.quotient(Jp, Jy)
    dtheta = rng.normal(size=(4, 18))
    dp = rng.normal(size=4)
    dT = (dp - (Jp[:, :18] * dtheta).sum(axis=1)) / Jp[:, 18]
    dy = (Jy[:, :18] * dtheta).sum(axis=1) + Jy[:, 18] * dT
    assert np.allclose(dy, (q[:, :18] * dtheta).sum(axis=1) + q[:, 18] * dp, rtol=1e-12, atol=1e-12)
