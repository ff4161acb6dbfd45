"""CPU: the referee of GcPcSaftMix.henrys_law_constant (tests/tools/gc_henry_referee.py) on its own: the input set stays within
the cap and every kept row has a finite twin, the gradient formula agrees with central differences of the referee's own ln H,
and the four k_ab records get a non-zero exact gradient for either solute (on the pure line they are exactly zero)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import gc_henry_referee as ref  # noqa: E402
import gc_point_rows as gp  # noqa: E402

SOLUTES = (0, 1)


def test_input_set_stays_within_the_cap(oracle):
    h = ref.inputs(oracle)
    c = h.c
    assert h.n == 3072
    worst = max(h.dropped_share.values())
    assert len(h.cells) == len(c.classes) * 2 * len(ref.sref.FACTORS)
    assert worst <= ref.CAP, h.dropped_share
    for s in SOLUTES:
        mine = h.solute == s
        k = h.keep & mine
        assert mine.sum() == 1536
        slope = h.dlnh[k] * c.rho_l[k]
        print("solute %d: kept %d of %d rows; ln H [Pa] %.1f .. %.1f; d ln H / d ln rho_L %.1f .. %.1f; twin: mu_s within %.1e, "
              "ln H within %.1e" % (s, k.sum(), mine.sum(), h.ln_h[k].min(), h.ln_h[k].max(), slope.min(), slope.max(),
                                    np.abs(h.mu_s64[k] - h.mu_s[k]).max(), h.twin_lnh[k].max()))
        assert k.sum() >= 1300
        # the twin solves what the referee solves: every kept row has a bar
        assert np.isfinite(h.twin_lnh[k]).all() and np.isfinite(h.mu_s64[k]).all()
        assert np.isfinite(h.ln_h[k]).all() and np.isfinite(h.dlnh[k]).all()
    print("largest dropped share of a (class, solute, factor) cell: %.3f (cap %.2f)" % (worst, ref.CAP))


def test_gradient_formula_against_central_differences(oracle):
    """d ln H / d(T, phi_0, phi_1) of the docstring's formula against central differences of the referee's own solve at relative
    steps h and h/2.  Bar, the differences' own error: the change between the two steps (their truncation error, which falls by
    4 from h to h/2) plus the rounding of ln H -- 2e-14 of the solve's rho_L times the row's |d ln H / d ln rho_L|, and 2e-14 of
    ln H's own magnitude (~20) -- over the step."""
    h = ref.inputs(oracle)
    c = h.c
    pick = np.nonzero(h.keep)[0][7::97][:32]
    assert len(set(h.solute[pick])) == 2
    m, idx, sol, T = c.m, c.row[pick], h.solute[pick], c.T[pick]
    one = np.ones(len(pick))
    want = ref.gradient(m, idx, sol, T, c.rho_v[pick], c.rho_l[pick], c.p_sat[pick], c.dp_l[pick], h.dlnh[pick], one)[0]
    noise = 2e-14 * (np.abs(h.dlnh[pick] * c.rho_l[pick]) + 20.0)
    step0 = 2e-5
    worst = 0.0
    for column, name in ((2, "T"), (0, "phi_0"), (1, "phi_1")):
        diffs = []
        for step in (step0, 0.5 * step0):
            vals = []
            for sign in (1.0, -1.0):
                if column == 2:
                    s = ref.solve(m, idx, sol, T * (1.0 + sign * step))
                    dx = T * step
                else:
                    phi = np.array(m.phi)
                    phi[idx, column] *= 1.0 + sign * step
                    s = ref.solve(ref.sref.Rows(oracle, m.enc, phi), idx, sol, T)
                    dx = m.phi[idx, column] * step
                assert s["ok"].all()
                vals.append(s["ln_h"])
            diffs.append((vals[0] - vals[1]) / (2.0 * dx))
        d1, d2 = diffs
        bar = np.abs(d1 - d2) + noise / (0.5 * step0 * np.abs(dx / step))
        err = np.abs(want[:, column] - d2)
        scale = np.abs(want).max(axis=1)
        print("d ln H / d %s: largest |formula - difference| %.2e of the row's largest component (difference's own error %.2e)"
              % (name, (err / scale).max(), (bar / scale).max()))
        assert (err <= bar).all(), (name, (err / bar).max())
        worst = max(worst, float((err / scale).max()))
    assert worst <= 1e-6


@pytest.mark.parametrize("solute", SOLUTES)
def test_kab_records_get_a_gradient(oracle, solute):
    h = ref.inputs(oracle)
    c = h.c
    wt = ref.weighted(oracle, h, solute)
    rec = gp.kab_records({"enc": c.m.enc, "kab_list": c.kab_list}, wt["all"]["grad_kab"])
    print("solute %d: exact k_ab records of sum_i g_i ln H_i: %s" % (solute, rec))
    assert len(rec) == 4 and np.isfinite(rec).all() and (rec != 0.0).all()
    assert np.isfinite(wt["all"]["grad_seg"]).all()
    for v in wt["groups"].values():
        assert np.isfinite(v["row"]).all()
        mine = h.solute[v["rows"]]
        assert (mine == solute).all()
        # both phi columns and T carry a gradient (on the pure line the other molecule's phi has none)
        assert (np.abs(v["row"]) > 0.0).any(axis=0).all()
