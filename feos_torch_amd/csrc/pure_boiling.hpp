// Boiling (saturation) temperature of a pure-component parameter row at a given pressure, one row per lane (device only,
// fp64, strict IEEE): the T with p_sat(T) = p_spec, together with the saturated densities at that T.
//
//   bounds   critical_point() (pure_critical.hpp) gives (T_c, p_c, rho_c): a p_spec that is non-finite, <= 0 or >= p_c
//            fails at once, and T_c is the first upper bound of the bracket.  It is solved with and without a caller's
//            initial temperature: p_spec >= p_c then fails the same way whatever the start, and the caller's value only
//            replaces the first iterate.  A row whose critical-point solve fails starts from the estimate 1.28 eps m^0.45 of
//            that header and finds its bounds by bracketing alone.
//   coords   x = 1/T, y = ln p: the saturation line is nearly straight there, so Newton on f(T) = ln p_sat(T) - ln p_spec
//            converges in a few steps.  First iterate: the caller's, or the line through (T_c, p_c) with the
//            corresponding-states slope  ln(p / p_c) = BOIL_SLOPE_CS (1 - T_c / T)  (simple fluids; every other row has a
//            steeper line, so the iterate lies below the answer, where the VLE solve is at its best).
//   trial    a VLE solve at the trial temperature (boil_trial): the coupled Newton iteration (vle_step, pure_solver.hpp)
//            warm-started from the densities of the last solved trial when that lies within BOIL_WARM_DT of T, otherwise
//            -- and whenever the warm iteration does not end on an acceptable state -- the full fp64 solve: vle_fast<false>,
//            and the per-lane vle_robust on the lanes it hands on.  Tolerances: those of the density outputs of
//            pcs_pure_vle (TOL_L_RHO, TOL_V_RHO, pure_solver.hpp: liquid step 1e-8, vapour step 1e-6, update applied).
//   slope    d ln p* / dT at fixed densities is the Clapeyron slope (p* is stationary in both densities at equilibrium):
//            one temperature tangent at both densities (pure_a_dT, pure_solver.hpp) in boil_dlnp_dT.
//   bracket  T_lo = highest trial with p_sat < p_spec, T_hi = lowest trial with p_sat > p_spec or without an equilibrium.
//            Trials stay strictly inside the known bounds, so every trial tightens one of them.  A Newton iterate outside
//            (or none: no equilibrium at the trial) is replaced by the midpoint in 1/T; with one bound missing it is
//            limited to a factor BOIL_MAX_RATIO in T.  "No equilibrium" from a cold solve is a SOFT bound: the robust pass
//            can miss an equilibrium that exists; once T_lo is within BOIL_WARM_DT of it the same temperature is tried
//            again, warm-started from below, and only that verdict is final.
//   accept   the trial's VLE solve converged and |f| <= BOIL_TOL_F, or |f| <= BOIL_TOL_F_NOISE directly after a trial with
//            |f| <= BOIL_TOL_F_PREV (the Newton step from there lands within 1e-15 of the root: what is left is the
//            rounding of p_sat itself on ill-conditioned rows).  d ln p_sat / d ln T > 1 on a saturation line (4 to 25 on
//            the pure_batch distribution), so T is at least that factor better than f.
//   fails    (status 1) bad parameters or pressure, the iteration cap, or a bracket that closes to BOIL_CLOSED without a
//            solved trial inside: pressures between p_sat at the highest temperature the VLE solve answers (0.999 T_c and
//            a shrinking share above) and p_c.
// All loops are wave-uniform: per-lane done / fail flags, exit on __ballot.  A lane's arithmetic depends on its own row only.
#pragma once
#include "pure_critical.hpp"
#include "pure_solver.hpp"

namespace pcs {

constexpr int BOIL_MAX_IT = 40;
constexpr int BOIL_WARM_IT = 12;
constexpr double BOIL_SLOPE_CS = 5.4;
constexpr double BOIL_WARM_DT = 0.03;
constexpr double BOIL_MAX_RATIO = 2.0;
constexpr double BOIL_STEP_DOWN = 1.1;  // no equilibrium and no lower bound yet: T <- T / BOIL_STEP_DOWN
constexpr double BOIL_CLOSED = 1e-6;
constexpr double BOIL_TOL_F = 1e-12, BOIL_TOL_F_NOISE = 1e-11, BOIL_TOL_F_PREV = 1e-8;

struct BoilResult {
    double T, rho_v, rho_l;  // K, A^-3
    int iters;               // trials (outer iterations)
};

// One VLE solve at temperature T on the lanes with `on` (wave-uniform call; the others idle or discard).  warm: start the
// coupled Newton from (rl, rv).  rho_c > 0: the critical density, which separates the phases of an accepted warm result
// (close to T_c, where rho_V / rho_L -> 1); without it the acceptance of vle_fast (rho_V < 0.7 rho_L).  Returns true with
// rl, rv (update applied) and the reduced equal-area pressure p_star; false leaves them untouched.
PCS_DEV bool boil_trial(const double* q, double T, bool on, bool warm, double rho_c, double& rl, double& rv, double& p_star) {
    PureCoef<double> c;
    pure_coef<double>(c, q, T, false);
    bool ok = false;
    if (__ballot(on && warm) != 0ull) {
        bool active = on && warm, done = false;
        double l_ = rl, v_ = rv, ps = 0.0;
        for (int it = 0; it < BOIL_WARM_IT; it++) {
            if (active && !done) {
                const Eval l = pure_eval(c, l_), v = pure_eval(c, v_);
                const VleStep s = vle_step(l, v, l_, v_);
                bool good = gt0(l.dp) && gt0(v.dp) && is_finite_bits(s.p_corr) && is_finite_bits(s.dl) && is_finite_bits(s.dv);
                const double ln = l_ + s.dl, vn = v_ + s.dv;
                good = good && (ln > 0.0) && (vn > 0.0) && (vn < ln);
                if (!good) {
                    active = false;
                } else {
                    done = (fabs(s.dl) <= TOL_L_RHO * l_) && (fabs(s.dv) <= TOL_V_RHO * v_);
                    l_ = ln;
                    v_ = vn;
                    ps = s.p_corr;
                }
            }
            if (__ballot(active && !done) == 0ull) break;
        }
        const bool apart = rho_c > 0.0 ? (v_ < rho_c && rho_c < l_ && v_ < l_ * (1.0 - 1e-6)) : (v_ < 0.7 * l_);
        if (active && done && apart && vapour_is_physical(ps, v_)) {
            ok = true;
            rl = l_;
            rv = v_;
            p_star = ps;
        }
    }
    const bool full = on && !ok;
    if (__ballot(full) != 0ull) {
        VleResult r;
        r.rho_v = r.rho_l = r.p_star = 0.0;
        int st = vle_fast<false>(q, T, r, TOL_L_RHO, TOL_V_RHO);  // every lane of the wave; only `full` lanes use it
        if (full && st == ST_RETRY) st = vle_robust(c, r, TOL_L_RHO);
        if (full && st == ST_OK) {
            ok = true;
            rl = r.rho_l;
            rv = r.rho_v;
            p_star = r.p_star;
        }
    }
    return ok;
}

// d ln p_sat / dT [1/K] at fixed densities, p_sat = p* T kB/A^3 with p* = -(a_V/rho_V - a_L/rho_L + ln(rho_V/rho_L)) /
// (1/rho_V - 1/rho_L): column 8 of the vapour-pressure Jacobian (pure_jacobian<0>, pure_jacobian.hpp) over p_sat, from the
// temperature tangent of a alone.
PCS_DEV double boil_dlnp_dT(const double* q, double T, double rl, double rv, double p_star) {
    const TempTangent t = pure_a_dT(q, T, rl, rv);
    const double inv_v = 1.0 / rv, inv_l = 1.0 / rl;
    const double dps = -(t.aT_v * inv_v - t.aT_l * inv_l) / (inv_v - inv_l);
    return 1.0 / T + dps / p_star;
}

// p_spec [Pa]; t_init [K]: the caller's first iterate (use_init, wave-uniform) or ignored.  Returns 0 (solved) or 1.
PCS_DEV int boiling_temperature(const double* par, double p_spec, double t_init, bool use_init, BoilResult& out) {
    out.T = out.rho_v = out.rho_l = 0.0;
    out.iters = 0;
    bool fail = !crit_params_ok(par) || !is_finite_bits(p_spec) || !(p_spec > 0.0);
    if (use_init && !(is_finite_bits(t_init) && t_init > 0.0)) fail = true;
    double q[8];
    row_or_idle(q, par, fail);
    CritResult cr;
    const bool have_c = critical_point(q, 0.0, false, cr) == 0;
    double Tc = 1.28 * q[2] * pow(q[0], 0.45), rho_c = 0.0, ln_pc = 0.0;
    if (have_c) {
        Tc = cr.T;
        rho_c = cr.rho;
        const double pc = cr.p * cr.T * P_UNIT;
        if (!fail && !(p_spec < pc)) fail = true;
        ln_pc = log(pc);
    }
    const double ln_p = log(fail ? 1.0 : p_spec);
    // bracket in x = 1/T: x_hi belongs to T_hi (x_hi < x < x_lo)
    double x_hi = have_c ? 1.0 / Tc : 0.0, x_lo = 0.0;
    bool have_hi = have_c, have_lo = false;
    double x = have_c ? (1.0 - (ln_p - ln_pc) * (1.0 / BOIL_SLOPE_CS)) / Tc : 1.0 / (0.7 * Tc);
    if (fail) x = 1.0 / (0.7 * Tc);
    if (use_init && !fail && !(have_hi && !(1.0 / t_init > x_hi))) x = 1.0 / t_init;
    double rl = 0.0, rv = 0.0, T_warm = 0.0, f_prev = 1.0;
    double x_sf = 0.0;  // soft upper bound: lowest temperature at which a cold solve found no equilibrium
    bool have_sf = false;
    bool warm = false, done = false;
    for (int it = 0; it < BOIL_MAX_IT; it++) {
        const bool on = !fail && !done;
        const double T = 1.0 / x;
        const bool w = warm && fabs(T - T_warm) <= BOIL_WARM_DT * T_warm;
        double ps = 0.0;
        const bool ok = boil_trial(q, T, on, w, rho_c, rl, rv, ps);
        if (on) {
            out.iters = it + 1;
            double x_new = -1.0;  // no Newton iterate
            if (ok) {
                const double f = log(ps * T * P_UNIT) - ln_p;
                if (!is_finite_bits(f)) {
                    fail = true;
                } else if (fabs(f) <= BOIL_TOL_F || (fabs(f_prev) <= BOIL_TOL_F_PREV && fabs(f) <= BOIL_TOL_F_NOISE)) {
                    done = true;
                    out.T = T;
                    out.rho_v = rv;
                    out.rho_l = rl;
                } else {
                    if (f < 0.0) {
                        x_lo = x;
                        have_lo = true;
                        if (have_sf && !(x > x_sf)) have_sf = false;  // solved at the soft bound after all
                    } else {
                        x_hi = x;
                        have_hi = true;
                        have_sf = false;  // trials lie below the soft bound: it is above this one
                    }
                    const double s = boil_dlnp_dT(q, T, rl, rv, ps);
                    // Newton in x: df/dx = -T^2 s
                    if (gt0(s)) x_new = x + f / (T * T * s);
                    if (!is_finite_bits(x_new)) x_new = -1.0;
                    f_prev = f;
                    warm = true;
                    T_warm = T;
                }
            } else {
                // no equilibrium found.  After a warm start from a solved neighbour that is taken as final (T_hi); a cold
                // solve alone can miss an equilibrium that exists (vle_robust on strongly non-ideal rows), so its verdict
                // only holds until a warm start from below has been tried at the same temperature
                if (w) { x_hi = x; have_hi = true; have_sf = false; } else { x_sf = x; have_sf = true; }
                f_prev = 1.0;
            }
            if (!fail && !done) {
                const bool have_up = have_sf || have_hi;
                const double x_up = have_sf ? x_sf : x_hi;
                if (have_lo && have_up) {
                    if (!(x_new > x_up && x_new < x_lo)) {
                        if (have_sf && fabs(1.0 / x_sf - T_warm) <= BOIL_WARM_DT * T_warm) {
                            x_new = x_sf;  // within reach of a warm start: put the soft bound to the test
                        } else {
                            if (x_lo - x_up <= BOIL_CLOSED * x_up) fail = true;
                            x_new = 0.5 * (x_lo + x_up);
                        }
                    }
                } else if (have_up) {
                    if (!(x_new > x_up)) x_new = x * BOIL_STEP_DOWN;
                    x_new = fmin(x_new, x * BOIL_MAX_RATIO);
                } else {
                    if (!(x_new > 0.0 && x_new < x_lo)) x_new = x * (1.0 / BOIL_STEP_DOWN);
                    x_new = fmax(x_new, x * (1.0 / BOIL_MAX_RATIO));
                }
                x = x_new;
            }
        }
        if (__ballot(!fail && !done) == 0ull) break;
    }
    return (done && !fail) ? 0 : 1;
}

}  // namespace pcs
