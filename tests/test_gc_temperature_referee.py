"""CPU: the referee behind tests/test_gc_temperature_gpu.py (tests/tools/gc_temperature_referee.py) stands on its own.

  1. the cap: at most 10 % of the rows of any (class, factor, problem) cell of the input set are dropped in advance, and the
     set has more than one row of every class it claims;
  2. from both displaced starts (0.93 / 1.07 T_grid) the referee returns T_grid within 1e-12 relative, and the oracle's
     pressure at the returned T is p_spec within 1e-12;
  3. the referee's quotient dT/dp_spec = 1 / (dp/dT) (exact pressure gradient at fixed densities) equals central differences
     of the WHOLE referee solve in p_spec on a few rows per class.  Bar 1e-5 relative as tests/test_mix_temperature_referee.py:
     a relative step of 1e-4 leaves a truncation error of h^2 times a third-derivative ratio of order 10-100, i.e. <= 1e-6,
     and a rounding error of the solve (T to ~1e-13) over 2 h of ~1e-9.

Measured: 384 of 384 rows kept in all six (factor, problem) cells; classes 0, 1, 2, 3, 5, 6 with 48 / 139 / 93 / 64 / 9 / 31 rows.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import gc_temperature_referee as ref  # noqa: E402

PROBLEMS = (False, True)
name = lambda dew: "dew" if dew else "bubble"


def test_what_the_referee_judges_exists_with_the_documented_arguments():
    import inspect

    from feos_torch_amd import GcPcSaftMix, native

    for method, first in (("bubble_temperature", "liquid_molefracs"), ("dew_temperature", "vapor_molefracs")):
        assert list(inspect.signature(getattr(GcPcSaftMix, method)).parameters) == ["self", "pressure", first, "temperature", "check_stability"]
    assert list(inspect.signature(native.gc_bubble_dew_temperature).parameters) == [
        "table", "S", "rows", "phi", "pressure", "molefracs", "temperature", "dew", "want_iters", "order"]


@pytest.mark.parametrize("dew", PROBLEMS)
def test_cap_on_rows_dropped_in_advance(oracle, dew):
    c = ref.inputs(oracle, dew)
    print(name(dew), "dropped per (factor, class) cell:", {k: round(v, 3) for k, v in c.dropped_share.items()})
    print(name(dew), "rows per class:", {int(k): int((c.cls[: ref.N_ROWS] == k).sum()) for k in np.unique(c.cls)},
          "d ln p / d ln T: %.1f ... %.1f" % (c.dlnp_dlnT[c.keep].min(), c.dlnp_dlnT[c.keep].max()), "smallest p_spec %.1e Pa" % c.p_spec[c.keep].min())
    assert c.n == len(ref.FACTORS) * ref.N_ROWS == 1152
    assert len(np.unique(c.cls)) >= 6
    assert max(c.dropped_share.values()) <= ref.CAP, c.dropped_share


@pytest.mark.parametrize("dew", PROBLEMS)
def test_referee_returns_the_grid_temperature_from_displaced_starts(oracle, dew):
    c = ref.inputs(oracle, dew)
    rows = np.nonzero(c.keep)[0]
    for s in ref.STARTS[1:]:
        T, p, _ = ref.solve_temperature(oracle, c, rows, c.p_spec[rows], s * c.T[rows], dew)
        assert np.isfinite(T).all(), (s, int((~np.isfinite(T)).sum()))
        eT, ep = np.abs(T / c.T[rows] - 1.0), np.abs(p / c.p_spec[rows] - 1.0)
        print(name(dew), "start", s, "max |T/T_grid - 1| %.2e  max |p/p_spec - 1| %.2e" % (eT.max(), ep.max()))
        assert (eT <= 1e-12).all() and (ep <= 1e-12).all()


@pytest.mark.parametrize("dew", PROBLEMS)
def test_referee_quotient_equals_central_differences_of_the_solve(oracle, dew):
    c = ref.inputs(oracle, dew)
    rows = np.concatenate([np.nonzero(c.keep & (c.cls == k))[0][[0, 7, -1]] for k in np.unique(c.cls)])
    ps, T0 = c.p_spec[rows], c.T[rows]
    q = ref.quotient(c.grad_row[rows])
    h = 1e-4
    solve = lambda p_: ref.solve_temperature(oracle, c, rows, p_, T0, dew)[0]
    fd_p = (solve(ps * (1 + h)) - solve(ps * (1 - h))) / (2 * h * ps)
    ep = np.abs(fd_p / q[:, 2] - 1.0)
    print(name(dew), "dT/dp: max rel %.2e on %d rows" % (ep.max(), len(rows)))
    assert (q[:, 2] > 0).all()
    assert (ep <= 1e-5).all()
