// Bubble / dew TEMPERATURE of a gc-PC-SAFT row at a given pressure, one row per lane (device only, fp64): the outer
// iteration of mix_temperature.hpp (bubble_dew_temperature_loop: safeguarded Newton on ln p(T) - ln p_spec in 1/T, the
// MIXT_* bracket rules, forward-difference tangent, warm-started trials, the confirming cold trial, the same failure list
// including the retrograde dew branch, which is not served) on the gc model.  Two things differ from the binary mixture:
//   coefficients at T   gc_coef<double>(m.c, row, tb, phi0, phi1, T) on the row bytes and table staged in LDS;
//   the cold trial      what k_gc_bubble_dew runs without a work list (full caps, single pass), so that the temperature
//                       returned is the one at which pcs_gc_bubble_dew itself answers p_spec:
//                         bubble  plain form, then -- only after a failed liquid root -- the robust form, restarted in place
//                                 (bubble_dew_solve_sm_both);
//                         dew     pure-liquid fugacities on the one-variable evaluation (pure_fugacities_on_the_line) feeding
//                                 start(), no damped second Newton run (may_damp = false), the no-progress leash
//                                 GC_NO_PROGRESS_DEW, and the robust form only after a failed liquid root.
// The warm trial is the Newton stage from the last solved trial's densities under the same two settings; where it does not
// end in BD_OK the lane goes on to the cold trial.
#pragma once
#include "gc_kernel_common.hpp"
#include "mix_solver_sm.hpp"
#include "mix_temperature.hpp"

namespace {

using namespace pcs;

// the settings of k_gc_bubble_dew on a lane that has just been started
template <bool DEW>
PCS_DEV void gc_lane_settings(BdLane<DEW>& L) {
    L.may_damp = false;
    if (DEW) L.np_limit = GC_NO_PROGRESS_DEW;
}

// One evaluation for every unfinished lane until all are done; a lane beyond its evaluation budget fails.  `restart`
// is asked once per lane that has ended without BD_OK and may start it again in place (returns true then).
template <bool DEW, class Model, class Restart>
PCS_DEV void gc_run_lanes(const Model& m, BdLane<DEW>& L, int guard_max, Restart restart) {
    int evals = 0;
    for (int guard = 0; guard < guard_max; guard++) {
        if (__ballot(!L.done()) == 0ull) break;
        if (L.done()) continue;
        double e0, e1;
        L.point(e0, e1);
        const PhaseEval e = phase_eval(m, e0, e1);
        L.consume(m, e);
        if (++evals >= (L.robust ? robust_eval_budget<DEW>() : BD_EVAL_GUARD) && !L.done()) L.idle();  // rc = BD_FAILED
        if (L.done() && L.rc != BD_OK && restart()) evals = 0;
    }
}

// One trial of the outer iteration at the model's temperature on the lanes with `on` (wave-uniform call; the others idle).
template <bool DEW, class Model>
PCS_DEV bool gc_temperature_trial(const Model& m, double z0, double p_init, bool on, bool warm, double rs, double ri0, double ri1,
                                  MixResult& out) {
    BdLane<DEW> L;
    L.idle();
    if (__ballot(on && warm) != 0ull) {
        if (on && warm) {
            L.start_newton(z0, p_init, rs, ri0, ri1, false);
            gc_lane_settings(L);
        }
        gc_run_lanes<DEW>(m, L, BD_EVAL_GUARD, [] { return false; });
    }
    const bool cold = on && !(warm && L.done() && L.rc == BD_OK);
    if (__ballot(cold) != 0ull) {
        double fug[2] = {-1.0, -1.0}, rho_pure[2] = {0.0, 0.0};
        if (DEW) pure_fugacities_on_the_line(m, fug, rho_pure);  // all lanes of the wave (2-4 one-variable evaluations)
        if (cold) {
            L.start(m, z0, p_init, SS_MAX_IT, NEWTON_MAX_IT, false, fug[0], fug[1], rho_pure[0], rho_pure[1]);
            gc_lane_settings(L);
        }
        gc_run_lanes<DEW>(m, L, BD_EVAL_GUARD + robust_eval_budget<DEW>(), [&] {
            if (L.robust || !L.root_failed) return false;
            L.start(m, z0, p_init, SS_MAX_IT, NEWTON_MAX_IT, true);
            gc_lane_settings(L);
            return true;
        });
    }
    const bool ok = on && L.done() && L.rc == BD_OK;
    if (ok) out = L.out;
    return ok;
}

// One gc row: tb / row are the table and the lane's row bytes in LDS, m.c.bond_dab / stride set by the caller.
template <bool DEW>
PCS_DEV int gc_temperature(GcModelT<double>& m, const unsigned char* row, const GcTable& tb, double phi0, double phi1, double z,
                           double p_spec, double t_init, bool fail, MixTempResult& out) {
    return bubble_dew_temperature_loop(
        m, p_spec, t_init, fail, out, [=, &m](double T) { gc_coef<double>(m.c, row, tb, phi0, phi1, T); },
        [=, &m](double T, bool on, bool warm, double rs, double ri0, double ri1, MixResult& r) {
            return gc_temperature_trial<DEW>(m, z, p_spec / (T * P_UNIT), on, warm, rs, ri0, ri1, r);
        });
}

}  // namespace
