// Per-lane density root of a binary mixture at given (T, p, x): the liquid-like or the vapour-like solution of
// p(x rho) = p_spec along the composition line rho_i = x_i rho (device only; see include/pcsaft_hip.h, pcs_mix_density).
//
// With a = line_eval (mix_solver.hpp: a, a', a'' along the line; inlined here, see line_eval_inline) the reduced quantities are
//     p(rho) = rho - a + rho a',      dp/drho = 1 + rho a''.
//
// The roots (eta = packing(x0, x1) rho):
//   liquid, rho_s = 0.5 / packing:
//     p(rho_s) >= p_spec: the largest rho <= rho_s with p = p_spec, provided dp/drho > 0 on all of [rho, rho_s]; where dp/drho
//                         reaches 0 first, the liquid branch ends above p_spec and the row fails;
//     p(rho_s) <  p_spec: the smallest rho > rho_s with p = p_spec, dp/drho > 0 and eta < DENS_ETA_MAX, else the row fails.
//     This is the root the bubble-point initialisation takes (S_ROOT, mix_solver_sm.hpp), converged to rounding.
//   vapour: the smallest rho > 0 with p = p_spec, provided dp/drho > 0 on (0, rho]; started at the ideal gas rho = p_spec
//           (at eta = DENS_ETA_VAPOUR where the ideal gas is denser than that).
//
// The iteration walks ALONG the branch from its start (rho_s downwards or upwards, the ideal gas upwards) and never
// bisects an interval it has not entered that way: a midpoint of (0, rho_s) may lie on the other branch, where "dp > 0 and
// not yet at p_spec" holds as well, and the walk would go on there.  State: `near`, the last point on the branch before
// the root (dp > 0, p on the start's side of p_spec), and, once a point has been past the root or past the end of the
// branch (dp <= 0), `far`, the closest such point.  Without `far` the next point is the Newton step from `near`, cut to
// DENS_WALK_DOWN / DENS_WALK_UP times the density (DENS_WALK_ETA in packing fraction above rho_s): a van der Waals loop
// narrower than that is the only thing a step can jump.  With `far` it is the Newton step where that falls strictly inside
// (near, far) and dp > 0, else the midpoint.  The liquid's Newton step is that of S_ROOT, on p (1 - eta)^4.  One loop, ONE
// evaluation site, bounded by DENS_MAX_EVALS.
//
// `Model` as in mix_solver.hpp: a coefficient struct with a<R>(r0, r1) and packing(x0, x1).
#pragma once
#include <stdint.h>

#include "mix_solver.hpp"

namespace pcs {

constexpr double DENS_ETA_START = 0.5;   // the liquid walk starts here (as S_ROOT)
constexpr double DENS_ETA_MAX = 0.74;    // close packing: no liquid root is taken at or above it
constexpr double DENS_ETA_VAPOUR = 0.05; // the vapour walk starts at the ideal gas or here, whichever is less dense (see density_root)
constexpr double DENS_WALK_DOWN = 0.8;   // largest step of the liquid walk down the branch (the factor of S_ROOT's robust form)
constexpr double DENS_WALK_UP = 1.25;    // largest step of the vapour walk up the branch
constexpr double DENS_WALK_ETA = 0.06;   // largest step, in packing fraction, of the liquid walk above eta = 0.5 (S_ROOT: 0.5 -> 0.62 -> ...)
// a row is accepted when the Newton step is below DENS_TOL rho, or has stopped shrinking (ratio >= 0.25) below DENS_FLOOR rho:
// the rounding floor of p / (dp/drho), the rule of NEWTON_FLOOR
constexpr double DENS_TOL = 1e-14;
constexpr double DENS_FLOOR = 1e-12;
// a bracket (near, far) whose far end lies past the END of the branch and that has closed to this relative width has found
// the spinodal, not a root: the row fails (p_spec is within ~1e-12 of the branch's last pressure, or beyond it)
constexpr double DENS_END_TOL = 1e-6;
// hard cap on evaluations per row (status 1 beyond it).  Converging rows of the 1e6-row synthetic batch need 3 - 9 (liquid) and
// 1 - 10 (vapour); rows that fail take the walk plus ~20 bisections towards the spinodal (DENS_END_TOL); a bracket closed by
// bisection alone would need ~47: see DESIGN.md section 4l for the histogram
constexpr int DENS_MAX_EVALS = 64;

enum : int { DENS_LIQUID = 0, DENS_VAPOUR = 1 };

// line_eval (mix_solver.hpp) for a kernel with ONE evaluation site: inlined, as phase_eval_inline is for the work-queue
// kernels, so that the model coefficients stay in registers / AGPRs instead of being read back from the caller's stack
// frame by the call (k_mix_density: 512 -> 24 B of scratch per lane).  A second call site would undo that: use line_eval then.
template <class Model>
PCS_DEV D2<double> line_eval_inline(const Model& m, double x0, double x1, double rho) {
    typedef D2<double> R;
    return m.template a<R>(R(x0 * rho, x0, 0.0), R(x1 * rho, x1, 0.0));
}

struct DensityResult {
    double rho, dpdrho;
    int evals;
};

// 0: converged (r filled); 1: failed.  x0 in [0, 1], p_spec > 0 finite (the caller has checked the row).
template <class Model>
PCS_DEV int density_root(const Model& m, int phase, double x0, double p_spec, DensityResult& r) {
    const double x1 = 1.0 - x0;
    const double pk = m.packing(x0, x1);
    const bool liquid = phase == DENS_LIQUID;
    // the ideal gas, unless that is denser than DENS_ETA_VAPOUR: far above the vapour branch rho = p_spec lies at liquid
    // densities, where "dp > 0, p < p_spec" holds as well.  On a vapour branch p < rho, so a p_spec the branch reaches is below
    // its spinodal density and the ideal gas is a point of the branch; a start cut to DENS_ETA_VAPOUR is either on the branch
    // or past its end (dp <= 0, and the bracket (0, start) then closes on the spinodal): liquid-like densities begin above it
    double rho = liquid ? DENS_ETA_START / pk : p_spec;
    if (!liquid && rho * pk > DENS_ETA_VAPOUR) rho = DENS_ETA_VAPOUR / pk;
    double near = liquid ? rho : 0.0, far = 0.0;
    bool have_far = false, far_ok = false;  // far_ok: far is past the ROOT on the branch (else past the branch's end)
    bool up = !liquid;                      // direction of the walk
    bool strict = true;                     // the branch ends where dp/drho <= 0 (not for the liquid walk above rho_s)
    double step_prev = 1e300;
    int nnewton = 0;
    r.rho = 0.0; r.dpdrho = 0.0; r.evals = 0;
    if (!(pk > 0.0) || !is_finite_bits(pk) || !is_finite_bits(rho)) return 1;
    for (int it = 0; it < DENS_MAX_EVALS; it++) {
        const D2<double> a = line_eval_inline(m, x0, x1, rho);
        const double p = rho - a.v + rho * a.d1, dp = 1.0 + rho * a.d2;
        const double f = p - p_spec;
        r.evals = it + 1;
        if (!is_finite_bits(p) || !is_finite_bits(dp)) return 1;
        if (liquid && it == 0) {
            up = f < 0.0;
            strict = !up;
            if (strict && !(dp > 0.0)) return 1;  // no liquid branch at eta = 0.5
        }
        const bool crossed = up ? f >= 0.0 : f <= 0.0;
        const bool on_branch = dp > 0.0 || !strict;
        if (!crossed && on_branch) {
            near = rho;
        } else {
            far = rho;
            have_far = true;
            far_ok = crossed && on_branch;
        }
        // Newton step from this point (liquid: on p (1 - eta)^4 as S_ROOT, plain where that has no positive slope)
        double den = dp;
        if (liquid) {
            const double scaled = dp - 4.0 * f * pk / (1.0 - rho * pk);
            if (scaled > 0.0) den = scaled;
        }
        const bool slope = dp > 0.0 && den > 0.0;
        double next = slope ? rho - f / den : -1.0;
        // a step below the tolerance ends the row wherever it points: next to the root it may round to nothing, or to just
        // outside a bracket that is a few doubles wide, and the bisection would then spend ~45 evaluations on closing it
        if (slope && fabs(next - rho) <= DENS_TOL * rho) {
            if (liquid && !(next * pk < DENS_ETA_MAX)) return 1;
            r.rho = next; r.dpdrho = dp;
            return 0;
        }
        bool newton;
        if (have_far) {
            const double lo = near < far ? near : far, hi = near < far ? far : near;
            newton = slope && next > lo && next < hi;
            if (!newton) next = 0.5 * (near + far);
            const double width = hi - lo;
            if (!newton && width <= DENS_TOL * hi) {  // closed by bisection
                if (!far_ok || !(dp > 0.0)) return 1;
                r.rho = next; r.dpdrho = dp;
                return 0;
            }
            if (!far_ok && width <= DENS_END_TOL * hi) return 1;  // the end of the branch, not a root
        } else {
            // the walk: rho is `near`
            newton = slope;
            if (up) {
                double cap = liquid ? rho + DENS_WALK_ETA / pk : DENS_WALK_UP * rho;
                if (liquid) {
                    const double top = DENS_ETA_MAX / pk;
                    if (!(rho < top)) return 1;  // no root below close packing
                    if (cap > top) cap = top;
                }
                if (!slope || !(next < cap)) { next = cap; newton = false; }
            } else {
                const double cap = DENS_WALK_DOWN * rho;
                if (!slope || !(next > cap)) { next = cap; newton = false; }
            }
        }
        if (newton) {
            const double step = fabs(next - rho);
            nnewton++;
            if (step <= DENS_TOL * rho || (nnewton >= 3 && step < DENS_FLOOR * rho && step >= 0.25 * step_prev)) {
                if (liquid && !(next * pk < DENS_ETA_MAX)) return 1;
                r.rho = next; r.dpdrho = dp;
                return 0;
            }
            step_prev = step;
        } else {
            step_prev = 1e300;
        }
        rho = next;
    }
    return 1;  // the cap
}

}  // namespace pcs
