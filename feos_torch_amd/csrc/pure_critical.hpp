// Vapour-liquid critical point of a pure-component parameter row, one row per lane (device only, fp64, strict IEEE).
//
// With p / kT = rho - a + rho a' (pure_model.hpp) the critical point is the state (T_c, rho_c) with
//     F1 = p_rho    / kT = 1 + rho a''     = 0
//     F2 = p_rhorho / kT = a'' + rho a'''  = 0        and  p_rhorhorho / kT = 2 a''' + rho a'''' > 0.
// pure_coef / pure_a are instantiated with P = DN<double,2> (tangents in temperature and density) and R = D3<P>: ONE
// evaluation gives a .. a''' with their temperature derivatives, and a'''' as the density tangent of a''', i.e. F, the full
// 2x2 Jacobian dF/d(T, rho), p and dp/dT.  (J is triangular at the solution: dF1/drho = F2 = 0; its diagonal p_rhoT and
// p_rhorhorho is far from zero, so the conditions are well conditioned.)
//
// Which critical point.  Strongly polar parameter sets give the equation of state a second van-der-Waals loop at liquid-like
// densities (pure_solver.hpp::vapour_is_physical), with a critical point of its own.  That loop exists at low temperatures
// only: above the vapour-liquid critical temperature the pure-component PC-SAFT isotherm is mechanically stable at every
// density (checked on the pure_batch distribution from 1.05 to 3 T_c over 0.01 <= eta <= 0.7, tests/test_critical_referee.py).
// The solver therefore takes the critical point with the HIGHEST temperature: it brackets the temperature at which the last
// mechanically unstable state (dp/drho < 0, the spinodal of vle_robust's density scan) disappears from a grid of vapour-liquid
// packing fractions, from above, and starts Newton from the bracket and the grid's minimiser of dp/drho.
//
//   start   g(T) = min over eta in CRIT_ETA0 + k CRIT_DETA (k < CRIT_NGRID) of dp/drho  (D2<double> evaluations).  From
//           T = 0.95 * 1.28 eps m^0.45 (the non-polar fit; polar / associating rows lie up to 4x above it) or the caller's
//           initial temperature: multiply by CRIT_GROW while g < 0, divide while g >= 0 and no sub-critical temperature is
//           known, then CRIT_BISECT bisections: T within ~1 %, rho from the grid minimiser.
//   Newton  on (T, rho) with the exact Jacobian; a step is scaled back to at most CRIT_MAX_DT of T and CRIT_MAX_DRHO of rho.
//           Converged when the relative step is below CRIT_TOL_T and CRIT_TOL_RHO; the update is applied (quadratic
//           convergence: the returned point is converged to the square of that), and p_c = p + p_T dT at the last
//           evaluation (p is flat to third order in rho there).
//   fails   (status 1): non-finite or non-physical parameters (without entering the loops' work), a cap, an iterate outside
//           T > 0, 0 < eta < CRIT_ETA_MAX, a non-finite value, or a converged point with p_rhorhorho <= 0.
// All loops are wave-uniform: they run until __ballot(lane still working) == 0 or their compile-time cap.
#pragma once
#include "pure_model.hpp"

namespace pcs {

constexpr int CRIT_NGRID = 8;
constexpr double CRIT_ETA0 = 0.05, CRIT_DETA = 0.02;  // 0.05 .. 0.19: critical packing fractions lie in 0.07 .. 0.18
constexpr double CRIT_GROW = 1.2;
constexpr int CRIT_MAX_BRACKET = 40;  // 1.2^40 = 1.5e3 either way
constexpr int CRIT_BISECT = 4;
constexpr int CRIT_MAX_NEWTON = 30;
constexpr double CRIT_MAX_DT = 0.1, CRIT_MAX_DRHO = 0.25;
constexpr double CRIT_TOL_T = 1e-10, CRIT_TOL_RHO = 1e-8;
constexpr double CRIT_ETA_MAX = 0.7;

struct CritResult {
    double T, rho, p;  // K, A^-3, reduced pressure p / kT [A^-3]
    double p3;         // p_rhorhorho / kT
    int iters;         // Newton iterations (diagnostics)
};

// finite, and physically meaningful for the model: m, sigma, eps > 0; mu any; kappa, eps_ab, na, nb >= 0
PCS_DEV bool crit_params_ok(const double* par) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; k++) ok = ok && is_finite_bits(par[k]);
    ok = ok && par[0] > 0.0 && par[1] > 0.0 && par[2] > 0.0;
    ok = ok && par[4] >= 0.0 && par[5] >= 0.0 && par[6] >= 0.0 && par[7] >= 0.0;
    return ok;
}

// q = the row, or harmless parameters for the lanes that idle through the wave-uniform loops of a solver (fail)
PCS_DEV void row_or_idle(double q[8], const double* par, bool fail) {
#pragma unroll
    for (int k = 0; k < 8; k++) q[k] = fail ? (k < 3 ? (k == 0 ? 1.0 : (k == 1 ? 3.5 : 200.0)) : 0.0) : par[k];
}

// min over the packing-fraction grid of dp/drho at temperature T; rho_min: its minimiser.  NaN-safe: a non-finite value
// makes the result non-finite.
PCS_DEV double crit_min_dp(const double* par, double T, double& rho_min) {
    PureCoef<double> c;
    pure_coef<double>(c, par, T, false);
    const double r_ceta = 1.0 / c.ceta;
    double g = 0.0;
    bool bad = false;
#pragma unroll 1
    for (int k = 0; k < CRIT_NGRID; k++) {
        const double rho = (CRIT_ETA0 + k * CRIT_DETA) * r_ceta;
        const D2<double> a = pure_a<double, D2<double>>(c, D2<double>(rho, 1.0, 0.0));
        const double dp = 1.0 + rho * a.d2;
        bad = bad || !is_finite_bits(dp);
        if (k == 0 || dp < g) {
            g = dp;
            rho_min = rho;
        }
    }
    return bad ? __longlong_as_double(0x7ff8000000000000LL) : g;
}

// One evaluation of the critical conditions at (T, rho) with their Jacobian.
struct CritEval {
    double F1, F2;          // p_rho / kT, p_rhorho / kT
    double F1T, F1r, F2T, F2r;  // d/dT, d/drho  (F2r = p_rhorhorho / kT)
    double p, pT;           // p / kT and its temperature derivative at fixed density
};
PCS_DEV CritEval crit_eval(const double* par, double T, double rho) {
    typedef DN<double, 2> G;
    typedef D3<G> R;
    G gp[8], gT(T), gr(rho);
#pragma unroll
    for (int k = 0; k < 8; k++) gp[k] = G(par[k]);
    gT.e[0] = 1.0;
    gr.e[1] = 1.0;
    PureCoef<G> c;
    pure_coef<G>(c, gp, gT, false);
    const R a = pure_a<G, R>(c, R(gr, G(1.0), G(0.0), G(0.0)));
    const G F1 = 1.0 + gr * a.d2;
    const G F2 = a.d2 + gr * a.d3;
    const G p = gr - a.v + gr * a.d1;
    CritEval e;
    e.F1 = F1.v; e.F1T = F1.e[0]; e.F1r = F1.e[1];
    e.F2 = F2.v; e.F2T = F2.e[0]; e.F2r = F2.e[1];
    e.p = p.v; e.pT = p.e[0];
    return e;
}

// t_init: caller's initial temperature [K] (use_init) or ignored.  Returns 0 (converged) or 1.
PCS_DEV int critical_point(const double* par, double t_init, bool use_init, CritResult& out) {
    out.T = out.rho = out.p = out.p3 = 0.0;
    out.iters = 0;
    bool fail = !crit_params_ok(par);
    double q[8];
    row_or_idle(q, par, fail);
    double T = 0.95 * 1.28 * q[2] * pow(q[0], 0.45);
    if (use_init && !fail) {
        if (is_finite_bits(t_init) && t_init > 0.0) T = t_init; else fail = true;
    }
    // ---- bracket: lo = highest temperature seen with an unstable state on the grid, hi = lowest without ----------------
    double lo = 0.0, hi = 0.0, rho = 0.0;
    bool have_lo = false, have_hi = false;
    for (int it = 0; it < CRIT_MAX_BRACKET; it++) {
        const bool work = !fail && !(have_lo && have_hi);
        if (work) {
            double r;
            const double g = crit_min_dp(q, T, r);
            if (!is_finite_bits(g)) {
                fail = true;
            } else if (g < 0.0) {
                lo = T; have_lo = true; rho = r;
                if (!have_hi) T *= CRIT_GROW;
            } else {
                hi = T; have_hi = true;
                if (!have_lo) { T *= (1.0 / CRIT_GROW); rho = r; }
            }
        }
        if (__ballot(!fail && !(have_lo && have_hi)) == 0ull) break;
    }
    if (!(have_lo && have_hi)) fail = true;
    for (int it = 0; it < CRIT_BISECT; it++) {
        if (!fail) {
            const double mid = 0.5 * (lo + hi);
            double r;
            const double g = crit_min_dp(q, mid, r);
            if (!is_finite_bits(g)) fail = true;
            else if (g < 0.0) { lo = mid; rho = r; }
            else hi = mid;
        }
    }
    T = 0.5 * (lo + hi);
    // ---- Newton on (T, rho) ------------------------------------------------------------------------------------------------
    bool done = false;
    for (int it = 0; it < CRIT_MAX_NEWTON; it++) {
        if (!fail && !done) {
            const CritEval e = crit_eval(q, T, rho);
            const double det = e.F1T * e.F2r - e.F1r * e.F2T;
            double dT = -(e.F1 * e.F2r - e.F1r * e.F2) / det;
            double dr = -(e.F1T * e.F2 - e.F2T * e.F1) / det;
            if (!is_finite_bits(dT) || !is_finite_bits(dr) || !is_finite_bits(e.p) || !is_finite_bits(e.pT)) {
                fail = true;
            } else {
                const double s = fmax(fabs(dT) / (CRIT_MAX_DT * T), fabs(dr) / (CRIT_MAX_DRHO * rho));
                if (s > 1.0) { dT /= s; dr /= s; }
                done = fabs(dT) <= CRIT_TOL_T * T && fabs(dr) <= CRIT_TOL_RHO * rho;
                if (done) {
                    out.p = e.p + e.pT * dT;
                    out.p3 = e.F2r;
                }
                T += dT;
                rho += dr;
                out.iters = it + 1;
                const double d = q[1] * (1.0 - 0.12 * exp(-3.0 * q[2] / T));
                const double eta = rho * (FRAC_PI_6 * (q[0] * (d * d * d)));
                if (!(T > 0.0) || !(eta > 0.0) || !(eta < CRIT_ETA_MAX)) fail = true;
            }
        }
        if (__ballot(!fail && !done) == 0ull) break;
    }
    if (fail || !done || !(out.p3 > 0.0) || !is_finite_bits(out.p)) return 1;
    out.T = T;
    out.rho = rho;
    return 0;
}

// Vector-Jacobian product of (T_c [K], p_c [Pa], rho_c [kmol/m3]) w.r.t. the 8 parameters at the converged point, by the
// implicit-function theorem:  d(T_c, rho_c)/dtheta = -J^-1 dF/dtheta,  dp_c/dtheta = p_theta + p_T dT_c/dtheta  (p_rho = 0),
// in adjoint form: J^T lambda = w once, then g_theta = -lambda . dF/dtheta + gp p_theta.  The tangents come from D3<DN<2>>
// evaluations, two directions per pass (a single D3<DN<9>> evaluation, 40 doubles per value, would not fit the stack
// budget): pass 0 = (T, rho) gives J, p and p_T, passes 1-4 the parameters in pairs.
PCS_DEV void critical_point_vjp(const double* par, double T, double rho, double gT, double gp, double grho, double g[8]) {
    typedef DN<double, 2> G;
    typedef D3<G> R;
    double lam1 = 0.0, lam2 = 0.0, wp = 0.0;
#pragma unroll 1
    for (int pass = 0; pass < 5; pass++) {
        G x[8], xT(T), xr(rho);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            x[k] = G(par[k]);
#pragma unroll
            for (int j = 0; j < 2; j++) x[k].e[j] = (pass >= 1 && 2 * (pass - 1) + j == k) ? 1.0 : 0.0;
        }
        if (pass == 0) {
            xT.e[0] = 1.0;
            xr.e[1] = 1.0;
        }
        PureCoef<G> c;
        pure_coef<G>(c, x, xT, true);
        const R a = pure_a<G, R>(c, R(xr, G(1.0), G(0.0), G(0.0)));
        const G F1 = 1.0 + xr * a.d2;
        const G F2 = a.d2 + xr * a.d3;
        const G p = xr - a.v + xr * a.d1;
        if (pass == 0) {
            // p_c [Pa] = p T P_UNIT:  dp_c = P_UNIT (T p_theta + (T p_T + p) dT_c);  rho_c [kmol/m3] = rho / RHO_UNIT
            wp = gp * (P_UNIT * T);
            const double w1 = gT + gp * (P_UNIT * (T * p.e[0] + p.v));
            const double w2 = grho * (1.0 / RHO_UNIT);
            // J^T lambda = w,  J = [[F1T, F1r], [F2T, F2r]]
            const double det = F1.e[0] * F2.e[1] - F1.e[1] * F2.e[0];
            lam1 = (w1 * F2.e[1] - F2.e[0] * w2) / det;
            lam2 = (F1.e[0] * w2 - F1.e[1] * w1) / det;
        } else {
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const double val = -(lam1 * F1.e[j] + lam2 * F2.e[j]) + wp * p.e[j];
#pragma unroll
                for (int k = 0; k < 8; k++)
                    if (k == 2 * (pass - 1) + j) g[k] = val;
            }
        }
    }
}

}  // namespace pcs
