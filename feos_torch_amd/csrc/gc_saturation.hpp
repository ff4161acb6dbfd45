// Per-lane vapour-liquid equilibrium of ONE molecule of a two-molecule model taken as a pure fluid (device only; see
// include/pcsaft_hip.h, pcs_gc_pure_vle).  The pure fluid is the composition line x0 = 1 or x0 = 0 of the row's model:
// with a, a', a'' = line_eval (mix_solver.hpp) along it, exactly as in density_root (mix_density.hpp),
//     p(rho) = rho - a + rho a',      dp/drho = 1 + rho a'',      a' = the residual chemical potential of the pure fluid.
//
// The solve is vle_robust (pure_solver.hpp) followed by the polish of saturated_state (pure_enthalpy.hpp), restated over an
// evaluator rho -> Eval{a, p, dp} and the packing m.packing(x0, x1) in place of PureCoef's ceta.  The pure-component
// routines are NOT templated over the evaluator: they stay as they are, so that every pure kernel keeps its bits; what
// takes `Eval`s (vle_step, vapour_is_physical, gt0) and the constants are used from there.
//   1. zero-pressure liquid from eta = 0.5 by Newton, vapour guess rho_L exp(a'(rho_L)), pulled back onto the stable vapour
//      branch by halving;
//   2. where 1 does not apply: both spinodals by geometric scans and bisection, branch solves at the mean of the spinodal
//      pressures; a fluid without a loop (every T at or above the critical temperature) or with a non-positive vapour-spinodal
//      pressure fails;
//   3. coupled Newton on the equal-area pressure p* = -(f_V - f_L)/(v_V - v_L), f = a/rho + ln rho (vle_step), backtracking
//      onto the stable branches; accepted when the solution is not trivial, vapour_is_physical, and the eight halving probes
//      below rho_V are mechanically stable;
//   4. polish: further vle_step updates until both relative steps are below SAT_TOL_POLISH, at most SAT_POLISH_IT -- the
//      saturated liquid density is an output and it is not stationary -- and ONE closing evaluation at the final densities,
//      whose step is not applied: it gives dp/drho at the roots themselves (the backward pass of the liquid density divides
//      by it) and the second-order corrected pressure of that last step.
// Lane-serial throughout: no wave-uniform loop, a lane's arithmetic and its evaluation count depend on its own row only.
// The evaluation is the non-inlined line_eval: the solver has ~25 evaluation sites (mix_density.hpp, line_eval_inline).
#pragma once
#include <stdint.h>

#include "mix_solver.hpp"
#include "pure_solver.hpp"

namespace pcs {

constexpr int SAT_POLISH_IT = 3;            // ENTH_POLISH_IT of pure_enthalpy.hpp
constexpr double SAT_TOL_POLISH = 1e-10;    // ENTH_TOL_POLISH
constexpr double SAT_TOL_L = 1e-8;          // TOL_L_RHO: the liquid step at which the coupled Newton of step 3 stops

// rho -> Eval along the pure line of `m`; counts its evaluations
template <class Model>
struct PureLine {
    const Model& m;
    double x0, x1;
    int evals;
    PCS_DEV Eval at(double rho, double& mu_res) {
        const D2<double> a = line_eval(m, x0, x1, rho);
        evals++;
        Eval e;
        e.a = a.v;
        e.p = rho - a.v + rho * a.d1;
        e.dp = 1.0 + rho * a.d2;
        mu_res = a.d1;
        return e;
    }
    PCS_DEV Eval operator()(double rho) {
        double mu;
        return at(rho, mu);
    }
};

struct SatResult {
    double p_star;        // reduced equal-area pressure (second-order corrected, vle_step)
    double rho_v, rho_l;  // A^-3
    double dp_v, dp_l;    // reduced dp/drho at the two roots
};

// branch_solve / spinodal_bisect of pure_solver.hpp over the evaluator
template <class Ev>
PCS_DEV double sat_branch_solve(Ev& ev, double p_spec, double lo, double hi, double rho) {
    for (int it = 0; it < 60; it++) {
        const Eval e = ev(rho);
        if (e.p > p_spec) hi = rho; else lo = rho;
        double rho_new = gt0(e.dp) ? rho - (e.p - p_spec) / e.dp : -1.0;
        if (!(rho_new > lo && rho_new < hi)) rho_new = 0.5 * (lo + hi);
        const double diff = fabs(rho_new - rho);
        rho = rho_new;
        if (diff <= 1e-13 * rho) break;
    }
    return rho;
}

template <class Ev>
PCS_DEV double sat_spinodal_bisect(Ev& ev, double lo, double hi, bool dp_positive_at_lo) {
    for (int it = 0; it < 26; it++) {  // 2^-26 of the bracket: the spinodals only seed the branch solves
        const double mid = 0.5 * (lo + hi);
        const Eval e = ev(mid);
        if (gt0(e.dp) == dp_positive_at_lo) lo = mid; else hi = mid;
    }
    return 0.5 * (lo + hi);
}

// steps 1 - 3: vle_robust of pure_solver.hpp over the evaluator; pk = packing fraction per unit density
template <class Ev>
PCS_DEV int sat_robust(Ev& ev, double pk, VleResult& out, double tol_l) {
    double rl = 0.0, rv = 0.0;
    bool have_init = false;
    {
        double rho = ETA_START / pk;
        bool ok = true;
        for (int it = 0; it < 40; it++) {
            const Eval e = ev(rho);
            if (!gt0(e.dp) || !is_finite_bits(e.p)) { ok = false; break; }
            const double step = e.p / e.dp;
            const double rho_new = rho - step;
            if (!gt0(rho_new)) { ok = false; break; }
            const bool conv = fabs(step) <= 1e-8 * rho;
            rho = rho_new;
            if (conv) break;
        }
        if (ok) {
            double mu;
            const Eval e = ev.at(rho, mu);
            if (gt0(e.dp) && is_finite_bits(mu)) {
                rl = rho;
                rv = rl * exp(mu);
                for (int k = 0; k < 60; k++) {
                    const Eval v = ev(rv);
                    if (gt0(v.dp) && gt0(v.p) && rv < 0.5 * rl) { have_init = true; break; }
                    rv *= 0.5;
                }
            }
        }
    }
    if (!have_init) {
        double rho = ETA_START / pk, rho_stable = rho;
        bool found = false;
        for (int k = 0; k < 60; k++) {
            const Eval e = ev(rho);
            if (!gt0(e.dp)) { found = true; break; }
            rho_stable = rho;
            rho *= 0.9;
        }
        if (!found) return ST_FAILED;  // super-critical
        const double rho_sl = sat_spinodal_bisect(ev, rho, rho_stable, false);
        double rho_unstable = rho;
        found = false;
        for (int k = 0; k < 120; k++) {
            rho *= 0.8;
            const Eval e = ev(rho);
            if (gt0(e.dp)) { found = true; break; }
            rho_unstable = rho;
        }
        if (!found) return ST_FAILED;
        const double rho_sv = sat_spinodal_bisect(ev, rho, rho_unstable, true);
        const double p_sl = ev(rho_sl).p, p_sv = ev(rho_sv).p;
        if (!gt0(p_sv)) return ST_FAILED;
        const double p0 = 0.5 * ((p_sl > 0.0 ? p_sl : 0.0) + p_sv);
        const double hi = 0.6 / pk;
        rl = sat_branch_solve(ev, p0, rho_sl, hi, 0.5 * (rho_sl + hi));
        rv = sat_branch_solve(ev, p0, 0.0, rho_sv, 0.5 * rho_sv);
    }
    double err_prev = 1.0;
    for (int it = 0; it < 60; it++) {
        const Eval l = ev(rl);
        const Eval v = ev(rv);
        const VleStep s = vle_step(l, v, rl, rv);
        double dl = s.dl, dv = s.dv;
        double rl_new = rl + dl, rv_new = rv + dv;
        bool damped = false;
        for (int k = 0; k < 12; k++) {
            if (gt0(rl_new) && gt0(ev(rl_new).dp)) break;
            dl *= 0.5;
            rl_new = rl + dl;
            damped = true;
        }
        for (int k = 0; k < 12; k++) {
            if (gt0(rv_new) && gt0(ev(rv_new).dp)) break;
            dv *= 0.5;
            rv_new = rv + dv;
            damped = true;
        }
        const double err = fmax(fabs(dl) / rl * (TOL_STEP / tol_l), fabs(dv) / rv);
        rl = rl_new;
        rv = rv_new;
        out.rho_v = rv;
        out.rho_l = rl;
        out.p_star = s.p_corr;
        out.iters = it + 1;
        if (!is_finite_bits(rl) || !is_finite_bits(rv) || !is_finite_bits(err)) return ST_FAILED;
        const bool stagnated = it >= 3 && err < 1e-7 && err >= 0.25 * err_prev;
        err_prev = err;
        if (!damped && (err <= TOL_STEP || stagnated)) {
            if (!(rv < rl * (1.0 - 1e-6))) return ST_FAILED;  // trivial solution
            if (!vapour_is_physical(out.p_star, rv)) return ST_FAILED;
            // the vapour root must lie on the branch that starts at zero density: no mechanically unstable state below it
            double probe = rv;
            for (int k = 0; k < 8; k++) {
                probe *= 0.5;
                if (!gt0(ev(probe).dp)) return ST_FAILED;
            }
            return ST_OK;
        }
    }
    return ST_FAILED;
}

// 0: solved (r filled, evals = evaluations used); 1: failed.  component 0: the line x0 = 1, component 1: x0 = 0.
template <class Model>
PCS_DEV int pure_line_vle(const Model& m, int component, SatResult& r, int& evals) {
    PureLine<Model> ev{m, component == 0 ? 1.0 : 0.0, component == 0 ? 0.0 : 1.0, 0};
    const double pk = m.packing(ev.x0, ev.x1);
    evals = 0;
    if (!gt0(pk)) return 1;
    VleResult s;
    s.rho_v = s.rho_l = s.p_star = 0.0;
    s.iters = 0;
    int st = sat_robust(ev, pk, s, SAT_TOL_L);
    double rl = s.rho_l, rv = s.rho_v, p_star = s.p_star, dpl = 0.0, dpv = 0.0;
    if (st == ST_OK) {
        bool conv = false;
        for (int k = 0; k <= SAT_POLISH_IT; k++) {
            const Eval l = ev(rl), v = ev(rv);
            const VleStep u = vle_step(l, v, rl, rv);
            dpl = l.dp;
            dpv = v.dp;
            const double ln = rl + u.dl, vn = rv + u.dv;
            const bool trust = is_finite_bits(u.dl) && is_finite_bits(u.dv) && is_finite_bits(u.p_corr) && fabs(u.dl) < 0.1 * rl &&
                               fabs(u.dv) < 0.5 * rv && vn > 0.0 && vn < ln;
            if (!trust) break;  // not a Newton step to trust: the densities and the pressure before it stand
            p_star = u.p_corr;
            if (conv || k == SAT_POLISH_IT) break;  // the closing evaluation: its step is not applied
            conv = (fabs(u.dl) <= SAT_TOL_POLISH * rl) && (fabs(u.dv) <= SAT_TOL_POLISH * rv);
            rl = ln;
            rv = vn;
        }
        if (!(rv < rl * (1.0 - 1e-6)) || !vapour_is_physical(p_star, rv) || !gt0(dpl) || !gt0(dpv) || !gt0(rl) || !gt0(rv)) st = ST_FAILED;
    }
    evals = ev.evals;
    if (st != ST_OK) return 1;
    r.p_star = p_star;
    r.rho_v = rv;
    r.rho_l = rl;
    r.dp_v = dpv;
    r.dp_l = dpl;
    return 0;
}

}  // namespace pcs
