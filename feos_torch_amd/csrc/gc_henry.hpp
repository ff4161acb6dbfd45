// Henry's law constant of ONE molecule of a gc-PC-SAFT row at infinite dilution in the other, pure and saturated, molecule of
// the row (device only; see include/pcsaft_hip.h: pcs_gc_henry).  The contract of mix_henry.hpp on the gc model:
//
//   definition   with s the solute, v = 1 - s the solvent, rho_L the saturated liquid density of molecule v taken as a pure
//                fluid at T and mu_s = da/drho_s the residual chemical potential of the row's two-molecule model at the partial
//                densities rho_v = rho_L, rho_s = 0 (what pcs_gc_derivatives returns as mu):
//                    H = rho_L k_B T exp(mu_s)  =  rho_L [A^-3] T P_UNIT exp(mu_s)   [Pa]
//   stage 1      pure_line_vle (gc_saturation.hpp) on the solvent, unchanged: the polished densities, the equal-area pressure
//                and dp/drho at both roots, as pcs_gc_pure_vle(component = v) returns them.
//   stage 2      ONE phase_eval (mix_solver.hpp) at (rho_L, 0) / (0, rho_L): mu_s and the mixed second derivative
//                d mu_s / d rho_v, which the total derivative of H along the solvent's saturation line needs:
//                    dlnh_drho = d ln H / d rho_L = 1 / rho_L + d mu_s / d rho_v.
//                rho_s = 0 is an ordinary point of the model: no logarithm of a partial density is taken.
// The two stages are separate __noinline__ functions, as in mix_henry.hpp: the solver's frame and the two-variable evaluation
// are then never live together.  Stage 2 is the kernel's only two-variable evaluation site and takes it inlined
// (phase_eval_inline, not the call phase_eval): by the compiler's resource report the call costs a second frame, 900 against
// 676 B of scratch per lane at the same 248 VGPRs (figures at the head of gc_henry.hip).  Lane-serial throughout: a lane's
// arithmetic depends on its own row only.
//
// `Model`: GcModelT<double> (gc_model.hpp).
#pragma once
#include "gc_saturation.hpp"

namespace pcs {

// stage 1: the pure solvent v of the row; true = solved
template <class Model>
__device__ __attribute__((noinline)) bool gc_henry_solvent(const Model& m, int v, SatResult& r, int& evals) {
    return pure_line_vle(m, v, r, evals) == 0;
}

// stage 2: (mu_s, d mu_s / d rho_v) at rho_v = rho_l, rho_s = 0
template <class Model>
__device__ __attribute__((noinline)) void gc_henry_solute(const Model& m, int solute, double rho_l, double& mu_s, double& dmu_drho) {
    const PhaseEval e = phase_eval_inline(m, solute == 0 ? 0.0 : rho_l, solute == 0 ? rho_l : 0.0);  // the only T2 site of the kernel
    mu_s = solute == 0 ? e.g0 : e.g1;
    dmu_drho = e.h01;
}

}  // namespace pcs
