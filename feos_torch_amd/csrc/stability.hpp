// Tangent-plane stability analysis of a binary feed state (device only; one row per lane).
//
// Feed: T and partial densities rho^f -> p^f, mu^f_i = ln rho^f_i + da/drho_i (reduced units of mix_solver.hpp).
// Trial phase: partial densities rho^t at the same T and pressure, on a mechanically stable root (dp/drho > 0 along its
// composition w).  tpd(rho^t) = sum_i w_i (mu_i(rho^t) - mu^f_i) [kT per mole of trial phase]; a feed is stable when no
// non-trivial trial phase has tpd < -TPD_TOL.  Outcome per row (include/pcsaft_hip.h, pcs_mix_stability):
//   STAB_STABLE    no stationary point of the search has tpd < -TPD_TOL; tpd = the smallest non-trivial one (+inf: none);
//   STAB_UNSTABLE  one has: tpd and rho^t of the smallest;
//   STAB_LOCAL     the Hessian of a + sum rho_i (ln rho_i - 1) is not positive definite at the feed (tpd = -inf, no search);
//   STAB_INVALID   non-finite or non-positive density, or p^f <= 0 (tpd = NaN).
//
// Search (Michelsen's successive substitution, written for two components): from a trial composition w with its root
// rho at p^f,  ln W_i = mu^f_i - da/drho_i(rho^t) - ln rho,  so the scalar s = ln(w_1/w_2) maps to
//     s' = (mu^f_1 - g_1) - (mu^f_2 - g_2),   F(s) = s' - s,   d tpd / ds = -w_1 w_2 F(s)
// (Gibbs-Duhem at fixed T and p): the substitution step s += F is a descent step of tpd along the branch, and its fixed
// points are the stationary points of tpd.  Where tpd is locally convex along the branch (F' < 0) the step is the Newton step
// -F / F', with F' from the Hessian of the one evaluation the substitution needs anyway (the branch derivative at constant
// p); elsewhere the plain substitution step.  Four deterministic starts: the ideal gas at the feed's chemical potentials
// (w_i ~ exp(mu^f_i)) on the vapour-like root, and liquid-like starts rich in either component and equimolar on the dense
// root (the equimolar one finds the second liquid of a split the incipient liquid of a dew point sits next to).
// Density roots of p(x rho) = p^f along the composition line (line_eval): safeguarded Newton with a bracket, entered from
// the dilute side (vapour-like) or from the first dense packing fraction of STAB_DENSE with p > p^f and dp > 0 (liquid-like),
// warm-started from the previous composition of the same start.  Every loop has a compile-time cap.
#pragma once
#include "mix_solver.hpp"

namespace pcs {

constexpr double TPD_TOL = 1e-8;       // a feed is unstable when a trial phase has tpd < -TPD_TOL
constexpr double TPD_TRIVIAL = 1e-6;   // |w_1 - z_1| and |rho^t / rho^f - 1| below this: the feed itself (never counts)
constexpr int STAB_ROOT_MAX_IT = 40;   // line evaluations per density root
constexpr int STAB_IT = 60;            // composition iterations per start
constexpr int STAB_BACKTRACK = 4;      // halvings of a composition step whose density root does not exist
constexpr double STAB_F_TOL = 1e-10;   // |F| at which a trial composition is stationary
constexpr double STAB_ROOT_TOL = 1e-12;  // relative Newton step at which a density root is accepted (the point returned carries it)
constexpr double STAB_S_MAX = 300.0;     // |ln(w_1/w_2)| bound (w ~ 5e-131: the incipient liquid of a dew point at 1e-30 bar can hold 1e-21)
constexpr double STAB_STEP_MAX = 4.0;    // largest change of s per iteration
constexpr int STAB_STARTS = 4;           // the vapour-like start and the liquid-like starts of STAB_S_LIQ
constexpr double STAB_S_LIQ[STAB_STARTS - 1] = {5.0, -5.0, 0.0};  // liquid-like starts: w = 0.9933, 0.0067, 0.5
constexpr double STAB_ETA_MAX = 0.7405;  // close packing: upper end of every bracket
constexpr int STAB_NDENSE = 4;
constexpr double STAB_DENSE[STAB_NDENSE] = {0.5, 0.6, 0.68, 0.72};  // packing fractions the dense root is entered from
enum : int { STAB_STABLE = 0, STAB_UNSTABLE = 1, STAB_LOCAL = 2, STAB_INVALID = 3 };

struct StabResult {
    double tpd, t0, t1;  // smallest tpd and the partial densities of its trial phase
    int status;
};

// p and dp/drho along rho_i = x_i rho
template <class Model>
PCS_DEV void stab_line_p(const Model& m, double x0, double x1, double rho, double& p, double& dp) {
    const D2<double> a = line_eval(m, x0, x1, rho);
    p = rho - a.v + rho * a.d1;
    dp = 1.0 + rho * a.d2;
}

// Root of p(x rho) = pf with dp/drho > 0 (0.0: none found).  liquid = false: entered from the dilute side (the start rho0,
// or the ideal-gas density pf, lies below the vapour-like root for an attractive fluid); true: from the dense side (rho0, or
// the first of STAB_DENSE with p > pf and dp > 0).  Bracket [lo, hi]: points on the far side of the wanted root in the
// direction of entry move the near end; a Newton step that leaves the bracket, or a point with dp <= 0, is replaced by
// bisection.
template <class Model>
PCS_DEV double stab_root(const Model& m, double x0, double x1, double pf, bool liquid, double rho0) {
    const double pk = m.packing(x0, x1);
    double lo = 0.0, hi = STAB_ETA_MAX / pk;
    double rho = rho0;
    if (!(rho > 0.0 && rho < hi)) {
        rho = pf;
        if (liquid) {
            rho = 0.0;
            for (int k = 0; k < STAB_NDENSE; k++) {
                const double r = STAB_DENSE[k] / pk;
                double p, dp;
                stab_line_p(m, x0, x1, r, p, dp);
                if (p > pf && dp > 0.0) { rho = r; break; }
                lo = r;  // p <= pf or mechanically unstable: the dense root lies above
            }
            if (rho == 0.0) return 0.0;
        } else if (!(rho < hi)) {
            rho = 0.5 * hi;
        }
    }
    for (int it = 0; it < STAB_ROOT_MAX_IT; it++) {
        double p, dp;
        stab_line_p(m, x0, x1, rho, p, dp);
        if (!is_finite_bits(p) || !is_finite_bits(dp)) return 0.0;
        const bool above = p > pf;
        if (liquid) {
            if (above && dp > 0.0) hi = rho; else lo = rho;
        } else {
            if (!above && dp > 0.0) lo = rho; else hi = rho;
        }
        double next;
        if (dp > 0.0) {
            const double step = (pf - p) / dp;
            next = rho + step;
            if (fabs(step) <= STAB_ROOT_TOL * rho) return next > 0.0 ? next : 0.0;
            if (!(next > lo && next < hi)) next = 0.5 * (lo + hi);
        } else {
            next = 0.5 * (lo + hi);
        }
        if (hi - lo <= 1e-14 * hi) return 0.0;  // shrunk onto a spinodal: no root on this side
        rho = next;
    }
    return 0.0;
}

// trial composition from s = ln(w_0 / w_1), without cancellation in the minor component
PCS_DEV void stab_comp(double s, double& w0, double& w1) {
    const double t = d_exp(-fabs(s));
    const double r = 1.0 / (1.0 + t);
    w0 = s >= 0.0 ? r : t * r;
    w1 = s >= 0.0 ? t * r : r;
}

template <class Model>
PCS_DEV StabResult stability_row(const Model& m, double r0, double r1) {
    const double nanv = __longlong_as_double(0x7ff8000000000000LL);
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    StabResult out;
    out.t0 = nanv;
    out.t1 = nanv;
    if (!(is_finite_bits(r0) && is_finite_bits(r1) && r0 > 0.0 && r1 > 0.0)) {
        out.tpd = nanv;
        out.status = STAB_INVALID;
        return out;
    }
    const PhaseEval f = phase_eval(m, r0, r1);
    const double pf = f.p();
    if (!(is_finite_bits(pf) && pf > 0.0)) {
        out.tpd = nanv;
        out.status = STAB_INVALID;
        return out;
    }
    // local test: Hessian of the Helmholtz energy density (ideal part included) in the partial densities
    const double H00 = f.h00 + 1.0 / r0, H11 = f.h11 + 1.0 / r1;
    if (!(H00 > 0.0 && H00 * H11 - f.h01 * f.h01 > 0.0)) {
        out.tpd = -inf;
        out.status = STAB_LOCAL;
        return out;
    }
    const double mu0 = f.mu0(), mu1 = f.mu1();
    const double rf = r0 + r1, z0 = r0 / rf;
    out.tpd = inf;
    for (int start = 0; start < STAB_STARTS; start++) {
        const bool liquid = start > 0;
        double s = start == 0 ? mu0 - mu1 : STAB_S_LIQ[start - 1];
        s = fmin(fmax(s, -STAB_S_MAX), STAB_S_MAX);
        double s_ok = s, rho_ok = 0.0;  // last composition whose root exists, and that root
        // bracket of a minimum: the last point with F > 0 (descent to the right) and the last one with F < 0
        double b_lo = -STAB_S_MAX, f_lo = 0.0, b_hi = STAB_S_MAX, f_hi = 0.0;
        bool has_lo = false, has_hi = false;
        int backtrack = 0;
        for (int it = 0; it < STAB_IT; it++) {
            double w0, w1;
            stab_comp(s, w0, w1);
            const double rho = stab_root(m, w0, w1, pf, liquid, rho_ok);
            if (rho == 0.0) {
                if (rho_ok == 0.0 || backtrack >= STAB_BACKTRACK) break;  // this start has no branch to follow
                backtrack++;
                s = 0.5 * (s + s_ok);
                continue;
            }
            backtrack = 0;
            const PhaseEval e = phase_eval(m, w0 * rho, w1 * rho);
            const double F = (mu0 - e.g0) - (mu1 - e.g1) - s;
            if (!is_finite_bits(F)) break;
            if (fabs(F) < STAB_F_TOL) {
                const bool trivial = fabs(w0 - z0) < TPD_TRIVIAL && fabs(rho / rf - 1.0) < TPD_TRIVIAL;
                if (!trivial) {
                    const double tpd = w0 * (e.mu0() - mu0) + w1 * (e.mu1() - mu1);
                    if (tpd < out.tpd) {
                        out.tpd = tpd;
                        out.t0 = e.r0;
                        out.t1 = e.r1;
                    }
                }
                break;
            }
            // F' = -d(g_0 - g_1)/ds - 1 along the branch at constant pressure
            const double dw = w0 * w1;
            const double d0 = e.dp0(), d1 = e.dp1();
            const double drho = -rho * dw * (d0 - d1) / (w0 * d0 + w1 * d1);
            const double dr0 = rho * dw + w0 * drho, dr1 = -rho * dw + w1 * drho;
            const double dF = -((e.h00 - e.h01) * dr0 + (e.h01 - e.h11) * dr1) - 1.0;
            double step = (dF < 0.0 && is_finite_bits(dF)) ? -F / dF : F;
            step = fmin(fmax(step, -STAB_STEP_MAX), STAB_STEP_MAX);
            if (fabs(s) >= STAB_S_MAX && s * step > 0.0) break;  // the descent leaves the composition range
            if (F > 0.0) { b_lo = s; f_lo = F; has_lo = true; } else { b_hi = s; f_hi = F; has_hi = true; }
            double next = fmin(fmax(s + step, -STAB_S_MAX), STAB_S_MAX);
            if (has_lo && has_hi && b_lo < b_hi && !(next > b_lo && next < b_hi)) {
                // the step leaves the bracket (a substitution step that overshoots by more than the distance to the
                // minimum, which otherwise ends in a 2-cycle): secant inside it, bisection if that fails
                next = b_lo - f_lo * (b_hi - b_lo) / (f_hi - f_lo);
                if (!(next > b_lo && next < b_hi)) next = 0.5 * (b_lo + b_hi);
            }
            s_ok = s;
            rho_ok = rho;
            s = next;
        }
    }
    out.status = out.tpd < -TPD_TOL ? STAB_UNSTABLE : STAB_STABLE;
    return out;
}

}  // namespace pcs
