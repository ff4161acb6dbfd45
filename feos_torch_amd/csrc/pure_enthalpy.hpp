// Enthalpy of vaporization of a pure-component parameter row at a given temperature, one row per lane (device only, fp64,
// strict IEEE), and its gradient along the saturation line.
//
//   definition   with a~ = a / rho (residual Helmholtz energy per molecule in kT), s(rho) = T a~_T + a~ + ln rho and the
//                saturated densities (rho_V, rho_L) at T:
//                    H = dh_vap / (R T) = s(rho_L) - s(rho_V)                                        (1)
//                    dh_vap [kJ/mol] = ENTH_UNIT T H,   ENTH_UNIT = 1e-6 RHO_UNIT P_UNIT  (= R in kJ/mol/K)
//   form         (1) IS the Clausius-Clapeyron form  (T / p*) (1/rho_V - 1/rho_L) (dp*/dT + p*/T)  with the equal-area pressure
//                p* = -(a~_V - a~_L + ln(rho_V / rho_L)) / (1/rho_V - 1/rho_L) of the VLE solve written out: the quotient by
//                the volume difference cancels, T dv dp*/dT = -T (a~_T,V - a~_T,L) and p* dv = -(a~_V - a~_L) - ln(rho_V / rho_L).
//                It is chosen over the direct form (-T a~_T + Z per phase) because it is the quantity the project already
//                differentiates: 1e-6 T dv times column 8 of the selector-0 Jacobian (pure_jacobian.hpp) at the same
//                densities, to rounding, and the referee of the tests (long-double Clapeyron slope) is the same formula.  The
//                two forms differ by (Z_V - Z_L) - p* dv, first order in the density error like the rest of either form
//                (H is not stationary in the densities: dH/drho = ds/drho != 0), and neither divides by the vanishing
//                volume difference near T_c once written as (1).  So the densities are converged further than the
//                density outputs of the VLE kernels need (ENTH_POLISH): exact coupled Newton updates (vle_step) after the solve
//                until the relative step is below ENTH_TOL_POLISH (the update is applied: the square of that is left), at
//                most ENTH_POLISH_IT; close to T_c, where dp/drho -> 0 amplifies the rounding of p, the cap ends it.
//   solve        the fp64 VLE solve that boil_trial (pure_boiling.hpp) runs cold: vle_fast<false>, then the per-lane
//                vle_robust on the lanes it hands on, with the density tolerances (TOL_L_RHO, TOL_V_RHO, pure_solver.hpp).
//   tangent      one temperature tangent at both densities (pure_a_dT, pure_solver.hpp).
//   fails        (status 1) non-finite or non-positive T, bad parameters (crit_params_ok), no equilibrium (every T >= T_c),
//                or a result that is non-finite or <= 0.
//   gradient     enthalpy_vjp: total derivative of dh_vap w.r.t. (8 parameters, T) along the saturation line.  The densities
//                respond to the parameters through F(rho_V, rho_L; theta, T) = (p_V - p_L, mu_V - mu_L) = 0 with
//                p / kT = rho - a + rho a', mu / kT = ln rho + a' (+ terms in T alone).  Adjoint form of the implicit-function
//                theorem, as critical_point_vjp:  J^T lambda = dH/d(rho_V, rho_L)  once, then
//                    dH/dx = H_x - lambda . F_x           for x in (theta_1..8, T),
//                J = [[p'_V, -p'_L], [p'_V / rho_V, -p'_L / rho_L]],  p' = 1 + rho a''  (plain D2<double> evaluations),
//                dH/drho_L = ds/drho (rho_L), dH/drho_V = -ds/drho (rho_V),
//                ds/drho = (T a'_T + a') / rho - (T a_T + a) / rho^2 + 1 / rho.
//                H_x and F_x need a, a', a_T, a'_T with their tangents in x: pure_coef / pure_a are instantiated with
//                P = D1<G> (the temperature as the one direction of D1) over G = DN<double, ENTH_CHUNK> (tangents in x) and
//                R = D1<P> (density direction).  The temperature is seeded in both levels when it is the direction x, so
//                a_TT arrives as the x-tangent of a_T and no second-order type is needed.  ENTH_CHUNK directions per pass,
//                both phases per pass in a loop that is not unrolled; the chunk width is what the stack budget of
//                tests/test_abi.py allows (a coefficient set is 33 P values = 66 (1 + ENTH_CHUNK) doubles).
// All loops are wave-uniform on __ballot; a lane's arithmetic depends on its own row only.
#pragma once
#include "pure_critical.hpp"
#include "pure_solver.hpp"

namespace pcs {

constexpr double ENTH_UNIT = 1e-6 * (RHO_UNIT * P_UNIT);
constexpr int ENTH_POLISH_IT = 3;
constexpr double ENTH_TOL_POLISH = 1e-10;
constexpr int ENTH_DIRS = 9;  // 8 parameters, T
#ifndef PCS_ENTH_CHUNK
#define PCS_ENTH_CHUNK 3
#endif
constexpr int ENTH_CHUNK = PCS_ENTH_CHUNK;

struct EnthalpyResult {
    double dh;            // kJ/mol
    double rho_v, rho_l;  // A^-3
};

// H = s(rho_L) - s(rho_V) at fixed densities (form (1) of the header)
PCS_DEV double enthalpy_reduced(const double* q, double T, double rl, double rv) {
    const TempTangent t = pure_a_dT(q, T, rl, rv);
    const double s_l = (T * t.aT_l + t.a_l) / rl, s_v = (T * t.aT_v + t.a_v) / rv;
    return (s_l - s_v) + log(rl / rv);
}

// The saturated state the enthalpy is taken at (`solve` and the polish of `form` in the header), shared with the Henry constant
// (mix_henry.hpp).  `bad`: the caller's own reasons to fail the row.  Returns fail; a failed lane idles through the wave-uniform
// loops on harmless values (row_or_idle) and its outputs are not to be used.  q: the row the solve ran on, T: its temperature,
// (rl, rv): the polished densities, p_star: the equal-area reduced pressure at them -- that of the last polish step with its
// second-order term (vle_step), or the solve's where no polish step was taken.  Wave-uniform call.
PCS_DEV bool saturated_state(const double* par, double T_in, bool bad, double q[8], double& T, double& rl, double& rv, double& p_star) {
    bool fail = bad || !crit_params_ok(par) || !is_finite_bits(T_in) || !(T_in > 0.0);
    row_or_idle(q, par, fail);
    T = fail ? 150.0 : T_in;
    VleResult r;
    r.rho_v = r.rho_l = r.p_star = 0.0;
    int st = vle_fast<false>(q, T, r, TOL_L_RHO, TOL_V_RHO);
    PureCoef<double> c;
    pure_coef<double>(c, q, T, false);
    if (st == ST_RETRY) st = vle_robust(c, r, TOL_L_RHO);
    if (st != ST_OK) fail = true;
    rl = fail ? 0.4 / c.ceta : r.rho_l;
    rv = fail ? 1e-3 * rl : r.rho_v;
    p_star = r.p_star;
    bool conv = fail;
    for (int k = 0; k < ENTH_POLISH_IT; k++) {
        if (!conv) {
            const Eval l = pure_eval(c, rl), v = pure_eval(c, rv);
            const VleStep s = vle_step(l, v, rl, rv);
            const double ln = rl + s.dl, vn = rv + s.dv;
            if (is_finite_bits(s.dl) && is_finite_bits(s.dv) && fabs(s.dl) < 0.1 * rl && fabs(s.dv) < 0.5 * rv && vn > 0.0 && vn < ln) {
                conv = (fabs(s.dl) <= ENTH_TOL_POLISH * rl) && (fabs(s.dv) <= ENTH_TOL_POLISH * rv);
                rl = ln;
                rv = vn;
                p_star = s.p_corr;
            } else {
                conv = true;  // not a Newton step to trust: the densities of the solve stand
            }
        }
        if (__ballot(!conv) == 0ull) break;
    }
    return fail;
}

// Returns 0 (solved) or 1.  Wave-uniform call.
PCS_DEV int enthalpy_of_vaporization(const double* par, double T_in, EnthalpyResult& out) {
    out.dh = out.rho_v = out.rho_l = 0.0;
    double q[8], T, rl, rv, p_star;
    const bool fail = saturated_state(par, T_in, false, q, T, rl, rv, p_star);
    const double dh = (ENTH_UNIT * T) * enthalpy_reduced(q, T, rl, rv);
    if (fail || !is_finite_bits(dh) || !(dh > 0.0)) return 1;
    out.dh = dh;
    out.rho_v = rv;
    out.rho_l = rl;
    return 0;
}

// g[0..7] = d dh_vap / d parameter, g[8] = d dh_vap / dT [kJ/mol per unit], along the saturation line, at the converged
// densities (rv, rl) of enthalpy_of_vaporization.  See the header comment.
PCS_DEV void enthalpy_vjp(const double* par, double T, double rv, double rl, double g[ENTH_DIRS]) {
    typedef DN<double, ENTH_CHUNK> G;
    typedef D1<G> P;
    typedef D1<P> R;
    constexpr int NPASS = (ENTH_DIRS + ENTH_CHUNK - 1) / ENTH_CHUNK;
    double dp[2];
    {
        PureCoef<double> c0;
        pure_coef<double>(c0, par, T, true);
        dp[0] = pure_eval(c0, rv).dp;
        dp[1] = pure_eval(c0, rl).dp;
    }
    const double rho[2] = {rv, rl};
    const double ln_lv = log(rl / rv);
#pragma unroll 1
    for (int pass = 0; pass < NPASS; pass++) {
        const int d0 = pass * ENTH_CHUNK;
        P x[8], xT;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            seed_unit(x[k].v, par[k], d0, k);
            x[k].d1 = G(0.0);
        }
        seed_unit(xT.v, T, d0, 8);
        xT.d1 = G(1.0);
        PureCoef<P> c;
        pure_coef<P>(c, x, xT, true);
        G H(0.0), F1(0.0), F2(0.0);
        double w[2];
#pragma unroll 1
        for (int ph = 0; ph < 2; ph++) {
            const double r = rho[ph], inv = 1.0 / r, sign = ph == 0 ? -1.0 : 1.0;
            const R a = pure_a<P, R>(c, R(P(r), P(1.0)));
            // a.v.v = a, a.v.d1 = a_T, a.d1.v = a', a.d1.d1 = a'_T, each with its tangents
            const G s = (xT.v * a.v.d1 + a.v.v) * inv;
            H = H + s * sign;
            F1 = F1 - (r - a.v.v + r * a.d1.v) * sign;
            F2 = F2 - a.d1.v * sign;
            w[ph] = sign * (((T * a.d1.d1.v + a.d1.v.v) - s.v) * inv + inv);
        }
        // J^T lambda = w
        const double uv = w[0] / dp[0], ul = -w[1] / dp[1];
        const double lam2 = (uv - ul) / (1.0 / rv - 1.0 / rl);
        const double lam1 = uv - lam2 / rv;
#pragma unroll
        for (int j = 0; j < ENTH_CHUNK; j++) {
            double val = (ENTH_UNIT * T) * (H.e[j] - (lam1 * F1.e[j] + lam2 * F2.e[j]));
            if (d0 + j == 8) val += ENTH_UNIT * (H.v + ln_lv);
#pragma unroll
            for (int d = 0; d < ENTH_DIRS; d++)
                if (d == d0 + j) g[d] = val;
        }
    }
}

}  // namespace pcs
