"""GPU: the fp32 pre-solve with lean coupled iterations (a and a' only, dp/drho carried by a secant; csrc/pure_f32.hpp).

A carried slope can go wrong where dp/drho -> 0 (near-critical rows: the quotient is noisy and the slope changes quickly),
where the vapour step is taken in ln(rho) (lowest temperatures, tiny p_sat) and where a step is so small that the quotient
of two fp32 pressures is rounding noise.  The rows: the 800 parameter rows of tests/tools/saturation_grid.py (all four
model classes) at T/T_c = 0.45, 0.6, 0.8, 0.9, 0.95, 0.99, 0.999 and the association-flag corner rows of
tests/test_pure_wave_mix_gpu.py, as one batch.

  * p_sat of the pressure-only kernel against the long-double oracle at the 1e-10 of tests/test_saturation_line_gpu.py
    (P_BAR), status identical to the oracle's mask;
  * the same for the pressure-only kernel handing out densities (k_pure_vle_rho) and the polished variant, densities at the
    bar of the saturation-line test (saturation_grid.bar);
  * the rows the main kernel hands to the all-fp64 fallback and to the robust pass are no more than the parent commit's
    (tests/golden/pure_lean_presolve_counts.json, measured on the same batch);
  * rows whose second coupled step is below 1e-5 relative (found with a CPU restatement of the coupled iteration on the
    oracle's derivatives): the lean iteration sees a secant of pure rounding noise there.

Mutation check (variant builds, MI355X): with the lean form forced on a lane's first coupled iteration 4 of the 6 tests
fail (p_sat up to 7.8e-10, fallback / robust lists 14 / 2,414 against the parent's 5 / 2,403); with the slopes handed to the
fp64 finish scaled by 1.1, 3 of 6 fail (p_sat 1.07e-10 at T/T_c 0.45, fallback list 6 against 5).
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import saturation_grid as sg  # noqa: E402
import test_saturation_line_gpu as saturation_line  # noqa: E402

pytestmark = pytest.mark.gpu

P_BAR = saturation_line.P_BAR  # the saturation-line test's bar for p_sat of every VLE variant
THETAS = (0.45, 0.6, 0.8, 0.9, 0.95, 0.99, 0.999)
N_CORNER = 4000
VARIANTS = ("vle_p", "vp_rho", "vle")  # k_pure_vle<true, false>, k_pure_vle_rho, k_pure_vle<true, true> (POLISH)
COUNTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pure_lean_presolve_counts.json")
PLAN_KINDS = {"pressure_only": {}, "rho_vl": {"want_rho_vl": True}}


def corner_rows(n=N_CORNER, seed=4244):
    """The association-flag corner rows of tests/test_pure_wave_mix_gpu.py::test_association_flag_corner_cases."""
    from feos_torch_amd.synthetic import pure_batch

    P, T = pure_batch(n, seed=seed)
    sites = (P[:, 6] != 0.0) | (P[:, 7] != 0.0)
    P = P.copy()
    k = np.arange(n) % 4
    P[sites & (k == 0), 4] = 0.0
    P[sites & (k == 1), 5] = 0.0
    P[sites & (k == 2), 6:8] = 0.0
    both0 = sites & (k == 3) & (np.arange(n) % 8 == 3)
    P[both0, 4] = 0.0
    P[both0, 5] = 0.0
    return P, T


def run_variant(name, P, T):
    from feos_torch_amd import native

    if name == "vle_p":
        r = native.pure_vle(P, T, want_rho_vl=False)
    elif name == "vp_rho":
        r = native.pure_vapor_pressure(P, T, want_rho_vl=True)
    else:
        r = native.pure_vle(P, T)
    out = {"status": r["status"].cpu().numpy().astype(bool), "p_sat": r["p_sat"].cpu().numpy()}
    if r["rho_vl"] is not None:
        rho = r["rho_vl"].cpu().numpy()
        out["rho_v"], out["rho_l"] = rho[:, 0].copy(), rho[:, 1].copy()
    return out


def main_kernel_counts(P, T):
    """{plan kind: [rows handed to the all-fp64 fallback, rows handed to the robust pass]} of the main kernel alone."""
    from feos_torch_amd import native

    out = {}
    for name, kind in PLAN_KINDS.items():
        plan = native.PureVlePlan(T.shape[0], T.device, **kind)
        plan.run_fast(P, T)
        torch.cuda.synchronize()
        out[name] = list(plan.retry_count())
    return out


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(oracle, hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    c = Ctx()
    g = sg.grid(orc=oracle)
    ref = sg.reference(orc=oracle)  # cached: shared with tests/test_saturation_line_gpu.py in one session
    sel = np.isin(g.theta, THETAS)
    assert sel.sum() == len(THETAS) * sg.N_ROWS
    c.theta = g.theta[sel]
    c.cond = ref["cond"]
    Pc, Tc = corner_rows()
    pc, stc = oracle.pure_vapor_pressure(Pc, Tc, prec=1)
    c.n_grid = int(sel.sum())
    c.P = np.ascontiguousarray(np.concatenate([g.P[sel], Pc]))
    c.T = np.ascontiguousarray(np.concatenate([g.T[sel], Tc]))
    ld = ref["ld"]
    c.want = {"p_sat": np.concatenate([ld["p_sat"][sel], pc]), "rho_v": ld["rho_v"][sel], "rho_l": ld["rho_l"][sel]}
    c.mask = np.concatenate([ld["st_p"][sel], stc])
    assert not c.mask[:c.n_grid].any()  # the oracle solves the whole grid up to 0.999
    c.Pd, c.Td = torch.from_numpy(c.P).cuda(), torch.from_numpy(c.T).cuda()
    c.res = {v: run_variant(v, c.Pd, c.Td) for v in VARIANTS}
    return c


@pytest.mark.parametrize("variant", VARIANTS)
def test_values_and_mask_against_the_long_double_oracle(ctx, variant):
    c, r = ctx, ctx.res[variant]
    bad = []
    diff = r["status"] != c.mask
    print("%s: status differs from the oracle's mask on %d rows (%d of them grid rows)" % (variant, diff.sum(), diff[:c.n_grid].sum()))
    if diff.any():
        bad.append(("mask", int(diff.sum()), np.flatnonzero(diff)[:8].tolist()))
    ok = ~r["status"] & ~c.mask
    for key in ("p_sat", "rho_v", "rho_l"):
        if key not in r:
            continue
        for th in THETAS + ("corner",):
            rows = np.arange(c.n_grid, len(c.T)) if th == "corner" else np.flatnonzero(c.theta == th)
            if th == "corner" and key != "p_sat":
                continue  # the density bars are defined on the saturation grid
            rows = rows[ok[rows]]
            err = np.abs(r[key][rows] / c.want[key][rows] - 1.0)
            e = float(err.max()) if len(err) else 0.0
            bar = P_BAR if key == "p_sat" else sg.bar(c.cond[key], th)
            print("values %-7s %-6s theta %-7s bar %.2e measured %.2e rows %d %s" % (variant, key, th, bar, e, len(rows), "" if e <= bar else "EXCEEDED"))
            if not e <= bar:
                bad.append((key, th, e, bar))
    assert not bad, bad


def test_p_sat_and_status_have_the_same_bits_with_and_without_densities(ctx):
    a, b = ctx.res["vle_p"], ctx.res["vp_rho"]
    assert np.array_equal(a["status"], b["status"])
    ok = ~a["status"]
    assert np.array_equal(a["p_sat"][ok].view(np.uint64), b["p_sat"][ok].view(np.uint64))


def test_fallback_and_robust_rows_not_more_than_the_parents(ctx):
    got = main_kernel_counts(ctx.Pd, ctx.Td)
    print("main-kernel lists (fallback, robust) now: %s" % got)
    with open(COUNTS) as f:
        parent = json.load(f)
    assert parent["rows"] == len(ctx.T)
    print("main-kernel lists (fallback, robust): parent %s: %s, now: %s" % (parent["commit"], parent["counts"], got))
    for kind in PLAN_KINDS:
        assert got[kind][0] <= parent["counts"][kind][0], (kind, "fallback", got[kind], parent["counts"][kind])
        assert got[kind][1] <= parent["counts"][kind][1], (kind, "robust", got[kind], parent["counts"][kind])


def coupled_steps_on_the_cpu(orc, P, T, n_it=2):
    """CPU restatement (fp64, the oracle's a, p, dp/drho) of the start of the pre-solve: zero-pressure liquid by the
    scaled Newton iteration from eta = 0.5 down to a 10 % step, vapour at the liquid's fugacity with the second-virial
    correction, then `n_it` coupled Newton iterations.  -> relative steps [n_it, n, 2] (liquid, vapour), valid mask."""
    m, sigma, eps = P[:, 0], P[:, 1], P[:, 2]
    d = sigma * (1.0 - 0.12 * np.exp(-3.0 * eps / T))
    ceta = np.pi / 6.0 * m * d ** 3
    valid = np.ones(len(T), dtype=bool)
    with np.errstate(all="ignore"):
        rl = 0.5 / ceta
        live = np.ones(len(T), dtype=bool)
        for it in range(12):
            a, p, dp = orc.pure_derivatives(P, T, rl)
            if it == 0:
                valid &= p > 0.0  # rows whose liquid lies above eta = 0.5 restart on the dense side: not followed here
            den = dp - 4.0 * p * ceta / (1.0 - rl * ceta)
            step = np.where(live, p / den, 0.0)
            valid &= ~live | ((den > 0.0) & (rl - step > 0.0))
            rl = np.where(valid, rl - step, rl)
            live &= ~(np.abs(step) <= 1e-1 * (rl + step))
        valid &= ~live
        al, pl, dpl = orc.pure_derivatives(P, T, rl)
        mu = (pl - rl + al) / rl
        rv = rl * np.exp(mu)
        tiny = 1e-6 * rv
        B = orc.pure_derivatives(P, T, tiny)[0] / tiny ** 2
        Lg, r = np.log(rv), rv.copy()
        for _ in range(3):
            den = np.maximum(1.0 + 2.0 * B * r, 0.3)
            r = r * np.maximum(1.0 - (np.log(r) + 2.0 * B * r - Lg) / den, 0.2)
        rv = np.where(np.isfinite(r) & (r > 0.0), r, rv)
        valid &= np.isfinite(rv) & (dpl > 0.0) & (rv < 0.5 * rl) & (rv > 1e-30)
        rl, rv = np.where(valid, rl, 0.4 / ceta), np.where(valid, rv, 1e-3 * 0.4 / ceta)
        steps = np.zeros((n_it, len(T), 2))
        for k in range(n_it):
            al, pl, dpl = orc.pure_derivatives(P, T, rl)
            av, pv, dpv = orc.pure_derivatives(P, T, rv)
            ps = -(av / rv - al / rl + np.log(rv / rl)) / (1.0 / rv - 1.0 / rl)
            dl, dv = -(pl - ps) / dpl, -(pv - ps) / dpv
            rln, rvn = rl + dl, rv + dv
            log_step = rvn < 0.3 * rv
            rvn = np.where(log_step, rv * np.exp(dv / rv), rvn)
            good = np.isfinite(rln) & np.isfinite(rvn) & (dpv > 0.0) & (dpl > 0.0) & (rvn > 1e-30) & (rvn < 0.6 * rln)
            valid &= good
            steps[k, :, 0], steps[k, :, 1] = np.abs(dl) / rl, np.abs(dv) / rv
            rl, rv = np.where(valid, rln, rl), np.where(valid, rvn, rv)
    return steps, valid, rl, rv


def test_rows_whose_second_coupled_step_is_rounding_noise(ctx, oracle):
    """Second coupled step below 1e-5 relative in both phases (and a first step that does not stop the lane): the p
    difference the secant divides is at the fp32 rounding level.  The rows must solve to the same bar."""
    from feos_torch_amd.synthetic import pure_batch

    c = ctx
    Pb, Tb = pure_batch(20_000, seed=515)
    P, T = np.concatenate([c.P, Pb]), np.concatenate([c.T, Tb])
    steps, valid, rl, rv = coupled_steps_on_the_cpu(oracle, P, T)
    first_goes_on = (steps[0, :, 0] > 2e-6) | (steps[0, :, 1] > 3e-5)
    noisy = valid & first_goes_on & (steps[1, :, 0] < 1e-5) & (steps[1, :, 1] < 1e-5)
    print("rows with a second coupled step below 1e-5: %d of %d (%d valid)" % (noisy.sum(), len(T), valid.sum()))
    assert noisy.sum() >= 200
    P, T = np.ascontiguousarray(P[noisy]), np.ascontiguousarray(T[noisy])
    want, st_o = oracle.pure_vapor_pressure(P, T, prec=1)
    rv_o, rl_o, st_v, _, _ = oracle.pure_vle(P, T, prec=1)
    # the restatement follows the iteration the kernel runs: two iterations in, it is at the oracle's root
    assert np.abs(rl[noisy] / rl_o - 1.0)[~st_v].max() < 1e-4 and np.abs(rv[noisy] / rv_o - 1.0)[~st_v].max() < 1e-4
    Pd, Td = torch.from_numpy(P).cuda(), torch.from_numpy(T).cuda()
    for variant in VARIANTS:
        r = run_variant(variant, Pd, Td)
        assert np.array_equal(r["status"], st_o), (variant, int((r["status"] != st_o).sum()))
        ok = ~st_o
        e = float(np.abs(r["p_sat"][ok] / want[ok] - 1.0).max())
        print("noisy secant %-7s p_sat bar %.1e measured %.2e rows %d" % (variant, P_BAR, e, ok.sum()))
        assert e <= P_BAR, (variant, e)
    fb, robust = main_kernel_counts(Pd, Td)["pressure_only"]
    print("noisy secant: fallback %d robust %d" % (fb, robust))
    # the rows reach their p_sat through the lean path under test, not through the all-fp64 fallback or the robust pass (a
    # row this close to its solution after one iteration is the main kernel's own; measured on the parent commit: 0 and 0)
    assert fb == 0 and robust == 0
