// Bubble / dew TEMPERATURE of a binary-mixture row at a given pressure and composition of the specified phase, one row per
// lane (device only, fp64): the T with p_bubble(T, z) = p_spec (resp. p_dew), with the partial densities of both phases at
// that T.  The mixture counterpart of pure_boiling.hpp; the inner solve is the bubble / dew state machine, unchanged.
//
//   coords   x = 1/T, y = ln p: the bubble and dew lines are nearly straight there, so Newton on
//            f(T) = ln p(T) - ln p_spec converges in a few steps from the caller's (mandatory) first iterate.
//   trial    mix_coef at T, then bubble_dew_trial_sm (mix_solver_sm.hpp) with the initial pressure p_spec: the first trial
//            is the cold solve of the single-pass kernel (plain form, robust second attempt); later trials start the Newton
//            stage from (rho_spec, rho_inc_1, rho_inc_2) of the last solved trial -- the composition of the specified phase
//            is fixed, so only its total density and the incipient phase move -- and fall back to the cold solve where that
//            does not end in BD_OK.  p(T) is the reference's final formula (feos_torch/pcsaft_mix.py:435-444) times T kB/A^3.
//   slope    d ln p / dT at fixed densities (the final formula is stationary in the densities at equilibrium, so this is the
//            slope of the bubble / dew line: column 18 of pcs_mix_jacobian over p): a one-direction temperature tangent of
//            the model as a forward difference -- the formula at T (1 + 2^-20) on two evaluations at the trial's densities
//            against the trial's pressure.  Its error (~1e-6 relative from the curvature, ~1e-7 from the rounding of p) only
//            enters the Newton step, never the result.  (The alternative, a secant through the last two solved trials, costs
//            no evaluation but has no slope after the first trial, one more trial per row on average, and its sign is noise
//            once two trials are 1e-13 apart -- which the retrograde test below cannot live with.)
//   bracket  T_lo = highest trial with p < p_spec, T_hi = lowest trial with p > p_spec or WITHOUT an equilibrium.  A Newton
//            iterate outside the known bracket is replaced by the midpoint in 1/T; with one bound missing the step is limited
//            to a factor MIXT_MAX_RATIO in T; a first iterate without an equilibrium is lowered by MIXT_STEP_DOWN at most
//            MIXT_MAX_DOWN times.
//   confirm  a trial accepted after a WARM start is repeated once, cold, at the same temperature.  Where the liquid can split
//            a vapour has two dew points (one per incipient liquid) and a liquid near the split more than one Newton basin;
//            warm starts follow the branch of the first trial, the cold solve of pcs_mix_bubble_dew picks its own.  The
//            confirmation makes the returned T the one at which pcs_mix_bubble_dew itself answers p_spec (the round trip
//            PcSaftMix.bubble_point(T) == p_spec): if the cold solve lands elsewhere the row goes on with cold trials only and
//            fresh bounds; if it finds nothing the warm-started solution stands.  Measured on the test set (576 rows per
//            problem, starts 7 % off): 5 dew rows started 7 % low change branch (up to 11 trials instead of 6); on 1e6 rows
//            started 5 % low the round trip misses 1e-9 on 1 bubble and 117 dew rows.  Cost: one cold solve per row.
//   accept   |f| <= MIXT_TOL_F, or |f| <= MIXT_TOL_F_NOISE directly after a trial with |f| <= MIXT_TOL_F_PREV (the two-trial
//            rule of BOIL_TOL_F_NOISE: the Newton step from there lands within 1e-15 of the root, what is left is the rounding
//            of the inner solve).  d ln p / d ln T > 1 on these lines, so T is at least that factor better than f.
//   fails    (status 1) a bad row (caller), a non-finite f, a solved trial whose slope is not positive and finite -- the
//            retrograde dew branch near a mixture critical point, where p falls with T, is NOT served --, no equilibrium at
//            the first iterate nor MIXT_MAX_DOWN steps below it, a bracket between a solved trial and one without an
//            equilibrium that closes to MIXT_CLOSED (p_spec above the highest pressure of the line), or MIXT_MAX_IT trials.
// All loops are wave-uniform: per-lane done / fail flags, exit on __ballot; every inner solve is bounded by the evaluation
// guards of the state machine.  A lane's arithmetic depends on its own row only.
#pragma once
#include "mix_model.hpp"
#include "mix_solver_sm.hpp"

namespace pcs {

constexpr int MIXT_MAX_IT = 40;
constexpr double MIXT_MAX_RATIO = 1.3;
constexpr double MIXT_STEP_DOWN = 1.1;
constexpr int MIXT_MAX_DOWN = 8;
constexpr double MIXT_CLOSED = 1e-6;
constexpr double MIXT_TOL_F = 1e-12, MIXT_TOL_F_NOISE = 1e-11, MIXT_TOL_F_PREV = 1e-8;
constexpr double MIXT_TANGENT_H = 1.0 / 1048576.0;  // relative temperature step of the tangent

struct MixTempResult {
    double T;     // K
    MixResult r;  // partial densities of both phases at T (A^-3)
    int iters;    // trials (outer iterations)
};

// The outer iteration, shared by the binary-mixture and the gc kernels (mix_temperature below, gc_temperature.hpp); the two
// differ in how the model is set to a temperature and in the cold solve of a trial, which come in as callables:
//   set_temperature(T)                                  the coefficients of m at T
//   trial(T, on, warm, rs, ri0, ri1, r) -> solved       one bubble / dew solve at the model's temperature on the lanes with `on`
//                                                       (wave-uniform call), warm-started from (rs, ri0, ri1) where `warm`
// m: the caller's model struct (left at an unspecified temperature).  fail: the row is bad -- the lane then carries a harmless
// row of the caller's through the wave-uniform code and takes no part in any solve.  Returns 0 (solved) or 1.
template <class Model, class SetT, class Trial>
PCS_DEV int bubble_dew_temperature_loop(Model& m, double p_spec, double t_init, bool fail, MixTempResult& out, SetT set_temperature,
                                        Trial trial) {
    out.T = 0.0;
    out.r.spec0 = out.r.spec1 = out.r.inc0 = out.r.inc1 = out.r.p = 0.0;
    out.r.iters = 0;
    out.iters = 0;
    const double ln_p = log(fail ? 1.0 : p_spec);
    // bracket in x = 1/T: x_hi belongs to T_hi (x_hi < x < x_lo)
    double x = 1.0 / (fail ? 300.0 : t_init), x_lo = 0.0, x_hi = 0.0;
    bool have_lo = false, have_hi = false, hi_solved = false;
    double rs = 0.0, ri0 = 0.0, ri1 = 0.0, f_prev = 1.0;
    bool warm = false, done = false, confirm = false, cold_only = false;
    int downs = 0;
    for (int it = 0; it < MIXT_MAX_IT; it++) {
        const bool on = !fail && !done;
        const double T = 1.0 / x;
        const bool use_warm = warm && !confirm && !cold_only;
        set_temperature(T);
        MixResult r;
        r.spec0 = r.spec1 = r.inc0 = r.inc1 = r.p = 0.0;
        r.iters = 0;
        const bool ok = trial(T, on, use_warm, rs, ri0, ri1, r);
        double s = 0.0;  // d ln p / dT
        if (__ballot(ok) != 0ull) {
            const double T2 = T * (1.0 + MIXT_TANGENT_H);
            set_temperature(T2);
            if (ok) {
                const PhaseEval es = phase_eval(m, r.spec0, r.spec1);
                const PhaseEval en = phase_eval(m, r.inc0, r.inc1);
                s = log((bubble_dew_formula(es, en) * T2) / (r.p * T)) / (T2 - T);
            }
        }
        if (on) {
            out.iters = it + 1;
            double x_new = -1.0;  // no Newton iterate
            if (ok) {
                const double f = log(r.p * T * P_UNIT) - ln_p;
                const bool accept = fabs(f) <= MIXT_TOL_F || (fabs(f_prev) <= MIXT_TOL_F_PREV && fabs(f) <= MIXT_TOL_F_NOISE);
                if (confirm && !accept) {
                    // the cold solve at the accepted temperature is on another branch (two incipient phases are possible where
                    // the liquid splits): what the warm starts have followed is not what pcs_mix_bubble_dew answers.  From here
                    // on every trial of the row is cold, and the bounds, which belong to the other branch, are dropped
                    cold_only = true;
                    have_lo = have_hi = hi_solved = false;
                }
                if (!is_finite_bits(f) || !is_finite_bits(s) || !(s > 0.0)) {
                    fail = true;
                } else if (accept) {
                    out.T = T;
                    out.r = r;
                    f_prev = f;
                    if (use_warm) confirm = true;  // same temperature once more, cold (`confirm` at the head of the file)
                    else done = true;
                } else {
                    if (f < 0.0) {
                        x_lo = x;
                        have_lo = true;
                    } else {
                        x_hi = x;
                        have_hi = true;
                        hi_solved = true;
                    }
                    x_new = x + f / (T * T * s);  // Newton in x: df/dx = -T^2 s
                    if (!is_finite_bits(x_new)) x_new = -1.0;
                    f_prev = f;
                    warm = true;
                    rs = r.spec0 + r.spec1;
                    ri0 = r.inc0;
                    ri1 = r.inc1;
                }
                if (!accept) confirm = false;
            } else if (confirm) {
                done = true;  // the cold solve finds nothing here: the warm-started solution stands
            } else {
                // no equilibrium at this trial: an upper bound on T
                x_hi = x;
                have_hi = true;
                hi_solved = false;
                f_prev = 1.0;
                if (!have_lo && ++downs > MIXT_MAX_DOWN) fail = true;
            }
            if (!fail && !done && !confirm) {
                if (have_lo && have_hi) {
                    if (!(x_new > x_hi && x_new < x_lo)) {
                        if (!hi_solved && x_lo - x_hi <= MIXT_CLOSED * x_hi) fail = true;
                        x_new = 0.5 * (x_lo + x_hi);
                    }
                } else if (have_hi) {
                    if (!(x_new > x_hi)) x_new = x * MIXT_STEP_DOWN;
                    x_new = fmin(x_new, x * MIXT_MAX_RATIO);
                } else {
                    if (!(x_new > 0.0 && x_new < x_lo)) x_new = x * (1.0 / MIXT_STEP_DOWN);
                    x_new = fmax(x_new, x * (1.0 / MIXT_MAX_RATIO));
                }
                x = x_new;
            }
        }
        if (__ballot(!fail && !done) == 0ull) break;
    }
    return (done && !fail) ? 0 : 1;
}

// Binary mixture: mix_coef at T, a trial is bubble_dew_trial_sm (mix_solver_sm.hpp).  m.c is filled from (par, k0, k1).
template <bool DEW, class Model>
PCS_DEV int mix_temperature(Model& m, const double* par, double k0, double k1, double z, double p_spec, double t_init, bool fail,
                            MixTempResult& out) {
    return bubble_dew_temperature_loop(
        m, p_spec, t_init, fail, out, [=, &m](double T) { mix_coef<double>(m.c, par, k0, k1, T); },
        [=, &m](double T, bool on, bool warm, double rs, double ri0, double ri1, MixResult& r) {
            return bubble_dew_trial_sm<DEW>(m, z, p_spec / (T * P_UNIT), on, warm, rs, ri0, ri1, r) == BD_OK;
        });
}

}  // namespace pcs
