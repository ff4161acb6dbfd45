// Henry's law constant of a solute at infinite dilution in a pure solvent, one binary-mixture row per lane (device only, fp64,
// strict IEEE; see include/pcsaft_hip.h: pcs_mix_henry).
//
//   definition   with s the solute, v the solvent, rho_L the saturated liquid density of the PURE solvent at T and
//                mu_s = da/drho_s the residual chemical potential of the binary model at the partial densities rho_v = rho_L,
//                rho_s = 0 (what pcs_mix_derivatives returns as mu):
//                    H = lim_{x_s -> 0} f_s / x_s = rho_L k_B T exp(mu_s)  =  rho_L [A^-3] T P_UNIT exp(mu_s)   [Pa]
//                the fugacity-based constant.  (The K-factor form y p / x differs by the solute's vapour-phase fugacity
//                coefficient; the kernel hands out rho_V and p_sat for a caller who wants it.)
//   stage 1      the solvent's saturated state exactly as the enthalpy of vaporization takes it (saturated_state,
//                pure_enthalpy.hpp: vle_fast<false>, vle_robust, polish to ENTH_TOL_POLISH).  H is NOT stationary in the
//                density -- d ln H / d ln rho_L reaches ~1e4 on the synthetic batch -- hence the polished density.
//   stage 2      ONE evaluation of the binary model at (rho_L, 0): phase_eval_inline (mix_solver.hpp), the T2 evaluation of
//                pcs_mix_derivatives.  It gives mu_s and the mixed second derivative d mu_s / d rho_v, which the total
//                derivative of H along the solvent's saturation line needs:
//                    dlnh_drho = d ln H / d rho_L = 1 / rho_L + d mu_s / d rho_v.
//                The pure limit rho_s = 0 is an ordinary point of the model (no logarithm of a partial density is taken here).
//   fails        (status 1, outputs 0) bad parameters of EITHER component (crit_params_ok), non-finite kij, non-finite or
//                non-positive T, no solvent equilibrium (every T >= T_c of the solvent), or an H that is non-finite or <= 0.
//                A supercritical solute is an ordinary row.
// The two stages are separate __noinline__ functions: the solver's frame and the mixture coefficients are then never live
// together (stack budget of tests/test_abi.py).  All loops are wave-uniform on __ballot (stage 1); a lane's arithmetic depends
// on its own row only.
//
// `Model`: MixModel of mix_kernel_common.hpp (coefficients c of mix_coef, a_z<R, Z>(r0, r1, zeta3), packing(x0, x1)).
#pragma once
#include "mix_model.hpp"
#include "mix_solver.hpp"
#include "pure_enthalpy.hpp"

namespace pcs {

struct HenryResult {
    double h;             // Pa
    double rho_v, rho_l;  // A^-3, the pure solvent's saturated densities
    double p_sat;         // Pa, the pure solvent's vapour pressure
    double dlnh_drho;     // A^3
};

struct HenrySolvent {
    double T, rho_v, rho_l, p_star;
    bool fail;
};

// stage 1: `bad` = the row's other reasons to fail (solute parameters, kij).  Wave-uniform call.
__device__ __attribute__((noinline)) HenrySolvent henry_solvent(const double* par_v, double T_in, bool bad) {
    HenrySolvent s;
    double q[8];
    s.fail = saturated_state(par_v, T_in, bad, q, s.T, s.rho_l, s.rho_v, s.p_star);
    return s;
}

// stage 2: (mu_s, d mu_s / d rho_v) at rho_v = rho_l, rho_s = 0
template <class Model>
__device__ __attribute__((noinline)) void henry_solute(const Model& m, int solute, double rho_l, double& mu_s, double& dmu_drho) {
    const PhaseEval e = phase_eval_inline(m, solute == 0 ? 0.0 : rho_l, solute == 0 ? rho_l : 0.0);
    mu_s = solute == 0 ? e.g0 : e.g1;
    dmu_drho = e.h01;
}

// Returns 0 (solved) or 1.  par: the row [2][8]; solute: 0 or 1 (wave-uniform).  Wave-uniform call.
template <class Model>
PCS_DEV int henry_constant(const double par[16], double k0, double k1, double T_in, int solute, HenryResult& out) {
    out.h = out.rho_v = out.rho_l = out.p_sat = out.dlnh_drho = 0.0;
    double pv[8];
#pragma unroll
    for (int k = 0; k < 8; k++) pv[k] = solute == 0 ? par[8 + k] : par[k];
    const bool bad = !crit_params_ok(par) || !crit_params_ok(par + 8) || !is_finite_bits(k0) || !is_finite_bits(k1);
    const HenrySolvent s = henry_solvent(pv, T_in, bad);
    if (s.fail) return 1;
    Model m;
    mix_coef<double>(m.c, par, k0, k1, s.T);
    double mu_s, dmu;
    henry_solute(m, solute, s.rho_l, mu_s, dmu);
    const double h = (s.rho_l * s.T * P_UNIT) * exp(mu_s);
    const double dl = 1.0 / s.rho_l + dmu;
    if (!is_finite_bits(h) || !(h > 0.0) || !is_finite_bits(dl)) return 1;
    out.h = h;
    out.rho_v = s.rho_v;
    out.rho_l = s.rho_l;
    out.p_sat = s.p_star * s.T * P_UNIT;
    out.dlnh_drho = dl;
    return 0;
}

}  // namespace pcs
