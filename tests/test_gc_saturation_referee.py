"""CPU: the referee of GcPcSaftMix.vapor_pressure / equilibrium_liquid_density (tests/tools/gc_saturation_referee.py) on its own:
the input set stays within the cap, the equilibrium conditions hold at the referee's solution, and its gradient formulas agree
with central differences of its own p_sat and rho_L."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import gc_saturation_referee as ref  # noqa: E402


def test_input_set_stays_within_the_cap(oracle):
    c = ref.inputs(oracle)
    assert c.n == 3072 and len(ref.FACTORS) == 4
    assert c.has_top.all(), "every (row, component) has an equilibrium on the ladder"
    worst = max(c.dropped_share.values())
    print("kept %d of %d rows; largest dropped share of a (class, component, factor) cell: %.3f (cap %.2f); T_top %.0f .. %.0f K"
          % (c.keep.sum(), c.n, worst, ref.CAP, c.t_top.min(), c.t_top.max()))
    assert len(c.cells) == len(c.classes) * 2 * len(ref.FACTORS)
    assert worst <= ref.CAP, c.dropped_share
    assert (c.dp_v[c.keep] >= ref.MIN_SLOPE).all() and (c.dp_l[c.keep] >= ref.MIN_SLOPE).all()
    # the twin solves what the referee solves: every kept row has a bar
    assert all(np.isfinite(v[c.keep]).all() for v in ref.twin_error(c).values())


def test_equilibrium_conditions_hold_at_the_solution(oracle):
    """p_V = p_L relative to max(p, p'_L rho_L) -- one ulp of the double rho_L moves p_L by 1e-16 p'_L rho_L, which is far more than
    1e-16 p on a cold liquid -- and mu_V + ln rho_V = mu_L + ln rho_L absolutely (both sides are of magnitude ~10): 1e-13."""
    c = ref.inputs(oracle)
    k = c.keep
    f1, f2 = np.abs(c.sol["f1"][k]).max(), np.abs(c.sol["f2"][k]).max()
    print("largest residuals at the referee's solution: pressure %.2e, chemical potential %.2e" % (f1, f2))
    assert f1 <= 1e-13 and f2 <= 1e-13
    assert (c.rho_v[k] < 0.7 * c.rho_l[k]).all() and (c.p_sat[k] > 0).all()
    # not an equilibrium between two dense states: a saturated vapour has 0 < Z <= 1
    assert (c.sol["p_star"][k] <= 1.0001 * c.rho_v[k]).all()
    # above T_top the referee finds nothing
    rows = np.nonzero(c.factor == 0)[0][::16]
    assert not ref.solve(c.m, c.row[rows], c.comp[rows], 1.5 * c.T_top[rows])["ok"].any()


def test_gradient_formulas_against_central_differences(oracle):
    """d p_sat / d(T, phi) and d rho_L / d(T, phi) of the docstring's formulas against central differences of the referee's own
    solve at relative steps h and h/2.  Bar, the differences' own error: the change between the two steps (their truncation
    error, which falls by 4 from h to h/2) plus the rounding of the solve, 2e-14 of the value, over the step."""
    c = ref.inputs(oracle)
    pick = np.nonzero(c.keep)[0][7::97][:32]
    m, idx, comp, T = c.m, c.row[pick], c.comp[pick], c.T[pick]
    n = len(pick)
    one = np.ones(n)
    want = {w: ref.gradient(m, idx, comp, T, c.rho_v[pick], c.rho_l[pick], c.p_sat[pick], c.dp_l[pick], one, w)[0] for w in (0, 1)}
    h = 2e-5
    worst = 0.0
    for column, name in ((2, "T"), (0, "phi_0"), (1, "phi_1")):
        diffs = []
        for step in (h, 0.5 * h):
            vals = []
            for sign in (1.0, -1.0):
                if column == 2:
                    s = ref.solve(m, idx, comp, T * (1.0 + sign * step))
                    dx = T * step
                else:
                    phi = np.array(m.phi)
                    phi[idx, column] *= 1.0 + sign * step
                    s = ref.solve(ref.Rows(oracle, m.enc, phi), idx, comp, T)
                    dx = m.phi[idx, column] * step
                assert s["ok"].all()
                vals.append((s["p_sat"], s["rho_l"]))
            diffs.append([(vals[0][w] - vals[1][w]) / (2.0 * dx) for w in (0, 1)])
        for w, value in ((0, c.p_sat[pick]), (1, c.rho_l[pick])):
            d1, d2 = diffs[0][w], diffs[1][w]
            bar = np.abs(d1 - d2) + 2e-14 * np.abs(value) / (0.5 * h * np.abs(dx / step))
            err = np.abs(want[w][:, column] - d2)
            scale = np.abs(want[w]).max(axis=1)
            print("d %s / d %s: largest |formula - difference| %.2e of the row's largest component (difference's own error %.2e)"
                  % ("p_sat" if w == 0 else "rho_L", name, (err / scale).max(), (bar / scale).max()))
            assert (err <= bar).all(), (w, name, (err / bar).max())
            worst = max(worst, float((err / scale).max()))
    assert worst <= 1e-6
