/*
 * pcsaft_hip.h — C ABI of libpcsaft_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the native half of feos-torch.  Each entry point replaces one method
 * of the reference's PyO3 classes (module `feos_torch.feos_torch`, src/lib.rs:10-16) together
 * with the per-row feos solve behind it, and additionally returns the property the reference's
 * Python tail computes from the converged densities (the kernels produce it in the same pass).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / torch tensor .data_ptr()), fp64 unless
 *     noted, C-contiguous; the caller owns all memory; nothing is allocated or freed here;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream) and
 *     the call returns without synchronising;
 *   - outputs are DENSE (length n): status[i] = 1 marks a row the solver could not converge
 *     (the reference drops such rows, src/pcsaft.rs:93-95; compaction is left to the caller);
 *   - optional outputs may be NULL;
 *   - return value 0 = enqueued, non-zero = API error, message via pcs_last_error();
 *   - parameter row layout (README.md:12): m, sigma[A], epsilon_k[K], mu[D], kappa_ab,
 *     epsilon_k_ab[K], na, nb.
 */
#ifndef PCSAFT_HIP_H
#define PCSAFT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Library / ABI version (major*100 + minor). */
int pcs_abi_version(void);

/* Last error message of the calling thread ("" if none). */
const char* pcs_last_error(void);

/* Bytes of device scratch a call on n rows needs (retry list of the pure / gc robust pass, or row order +
 * control block of the mixture work queue). */
int64_t pcs_workspace_bytes(int64_t n);

/*
 * Pure-component VLE at fixed temperature.
 * Replaces PcSaft.vapor_pressure(parameters[N,8], temperature[N]) -> (rho[n_ok,4], status[N])
 * (src/pcsaft.rs:18-26, :82-103) and the Python tails of PcSaftPure.vapor_pressure
 * (feos_torch/pcsaft_pure.py:201-215) and .equilibrium_liquid_density (:217-233).
 *   params   [n,8]   in
 *   temp     [n]     in   K
 *   p_sat    [n]     out  Pa            (optional)  pcsaft_pure.py:214-215
 *   rho_eq   [n]     out  kmol/m3       (optional)  pcsaft_pure.py:232-233
 *   rho_vl   [n,2]   out  A^-3: (rho_V, rho_L) at which the formulas were evaluated (optional;
 *                         the reference's rho[:,0:2] of src/pcsaft.rs:99-100)
 *   status   [n]     out  uint8, 1 = failed
 *   iters    [n]     out  int32, Newton iterations used (optional, diagnostics)
 *   workspace        device scratch of pcs_workspace_bytes(n)
 * Kernels: pressure only -- fp32 pre-solve + fp64 finish with the pre-solve's dp/drho; rho_vl -- the all-fp64 iteration from
 * the pre-solve's start (densities ~1e-11); rho_eq -- the pressure-only path + one exact fp64 Newton update of both densities
 * (~1e-14; p_sat then carries that step's second-order term).
 */
int pcs_pure_vle(const double* params, const double* temp, int64_t n, double* p_sat, double* rho_eq,
                 double* rho_vl, uint8_t* status, int32_t* iters, void* workspace, void* stream);

/*
 * The two stages of pcs_pure_vle as separate launches, same arguments (for per-kernel timing and
 * for callers that want to overlap the rare-row robust pass with other work):
 *   pcs_pure_vle_fast   zeroes the retry counter, runs the fast kernel on all n rows and appends
 *                       rows that need the robust initialisation to the workspace list;
 *   pcs_pure_vle_retry  runs the robust kernel over that list (count read on the device).
 * pcs_pure_vle == pcs_pure_vle_fast followed by pcs_pure_vle_retry on the same stream.
 */
int pcs_pure_vle_fast(const double* params, const double* temp, int64_t n, double* p_sat, double* rho_eq,
                      double* rho_vl, uint8_t* status, int32_t* iters, void* workspace, void* stream);
int pcs_pure_vle_retry(const double* params, const double* temp, int64_t n, double* p_sat, double* rho_eq,
                       double* rho_vl, uint8_t* status, int32_t* iters, void* workspace, void* stream);

/*
 * A reusable row order for the pressure-only fast stage (ABI 116).
 *   pcs_pure_row_order         writes order_out (int32[n]): the batch is cut into tiles of 16384 consecutive rows (the last one
 *                              may be short) and the entries of a tile are a permutation of that tile's row indices, ordered
 *                              by model class (none, polar, polar + associating, associating) and, inside a class, by the
 *                              sub-key of pcs_pure_order_key: the fp32 pre-solve is run on every row and the rows are binned
 *                              by how close it came to a third coupled iteration and a third liquid-root evaluation.  Two
 *                              kernels (order_out is the first one's scratch), no memset, no host synchronisation: capturable.
 *                              It costs about as much as one solve: for rows that are solved many times.
 *   pcs_pure_vle_fast_ordered  pcs_pure_vle_fast in its pressure-only form (rho_eq and rho_vl must be null) with lane t of
 *                              the kernel solving row order[t]: waves then hold rows of one class and similar iteration counts.
 * The order is a scheduling hint: rows are independent, so p_sat, status and the set of listed rows are bit for bit those
 * of pcs_pure_vle_fast whatever permutation is passed -- an order built from other parameters or temperatures (an earlier
 * step of a fit) costs speed only.  It must be a permutation of 0..n-1 for every row to be solved; entries are bounded by
 * n on the device, so a foreign array cannot fault.  pcs_pure_vle_retry follows as after pcs_pure_vle_fast.
 */
int pcs_pure_row_order(const double* params, const double* temp, int64_t n, int32_t* order_out, void* stream);
int pcs_pure_vle_fast_ordered(const double* params, const double* temp, int64_t n, double* p_sat, double* rho_eq,
                              double* rho_vl, uint8_t* status, int32_t* iters, void* workspace, const int32_t* order,
                              void* stream);

/*
 * Probe of the row order's key (ABI 119; tests and scripts/dev/k1_wave_stats.py): what pcs_pure_row_order sorts on, per row.
 *   key_out [n] int32    class * 64 + sub-key (class: none 0, polar 1, polar + associating 2, associating 3)
 *   raw_out [n,4] int32  what the fp32 pre-solve did on the row: liquid-root evaluations | coupled iterations << 8 |
 *                        failure code << 16 | flags << 24 (1: a full liquid, 2: a full vapour evaluation in a coupled
 *                        iteration >= 2) | usable << 31 (finite, positive inputs and a pre-solve that succeeded), then the
 *                        bits of three fp32 margins value / threshold of its stop decisions: the liquid root's second step,
 *                        the liquid and the vapour side of the second coupled iteration.
 */
int pcs_pure_order_key(const double* params, const double* temp, int64_t n, int32_t* key_out, int32_t* raw_out, void* stream);

/*
 * pcs_pure_vle with the all-fp64 main kernel (fp64 value / first / second derivative in every Newton iteration after the
 * fp32 start) whatever the outputs -- the validation twin of pcs_pure_vle: same arguments, same results to ~1e-11.
 */
int pcs_pure_vle_fp64(const double* params, const double* temp, int64_t n, double* p_sat, double* rho_eq,
                      double* rho_vl, uint8_t* status, int32_t* iters, void* workspace, void* stream);

/*
 * PcSaftPure.vapor_pressure as ONE call (feos_torch/pcsaft_pure.py:201-215 incl. its Rust solve, src/pcsaft.rs:82-103):
 * always the pressure-only kernel of pcs_pure_vle (fp32 pre-solve, fp64 finish), so p_sat carries the same bits whether
 * or not the caller also asks for the densities.
 *   rho_vl [n,2] out (optional) the densities the last fp64 Newton step of that kernel ended on: ~1e-9 (relative) from the
 *                root -- what the Jacobian kernel needs; p_sat is second order in that error.  For converged densities
 *                (the reference's rho output) call pcs_pure_vle with rho_vl.
 */
int pcs_pure_vapor_pressure(const double* params, const double* temp, int64_t n, double* p_sat, double* rho_vl,
                            uint8_t* status, void* workspace, void* stream);

/*
 * Liquid density at given (T, p).
 * Replaces PcSaft.liquid_density(parameters[N,8], temperature[N], pressure[N]) ->
 * (rho[n_ok], status[N]) (src/pcsaft.rs:28-41, :105-129) and the tail of
 * PcSaftPure.liquid_density (feos_torch/pcsaft_pure.py:184-199).
 *   pressure [n]  in   Pa
 *   rho_out  [n]  out  kmol/m3  (optional)  pcsaft_pure.py:198-199
 *   rho_root [n]  out  A^-3 converged density (the reference's rho of src/pcsaft.rs:127) (optional)
 */
int pcs_pure_liquid_density(const double* params, const double* temp, const double* pressure, int64_t n,
                            double* rho_out, double* rho_root, uint8_t* status, void* stream);

/*
 * (a, p, dp/drho) at given (T, rho) — PcSaftPure.derivatives (feos_torch/pcsaft_pure.py:180-182).
 * All reduced (A^-3).  Any output may be NULL.
 */
int pcs_pure_derivatives(const double* params, const double* temp, const double* rho, int64_t n, double* a,
                         double* p, double* dp, void* stream);

/*
 * Test probe of the fp32 pre-solve: the model evaluation its liquid root starts from (rho = 0.5 / ceta, packing fraction
 * 0.5), in fp32 as the kernels compute it.
 *   out [n,8] float  (a, p, dp/drho, a') from the generic evaluation, then the same four from the closed form at the
 *                    fixed packing fraction that the first iteration of the root uses.  All reduced (A^-3).
 */
int pcs_pure_start_probe(const double* params, const double* temp, int64_t n, float* out, void* stream);

/*
 * Jacobian of a pure-component property w.r.t. its inputs with the phase densities held
 * fixed — what torch reverse mode through the reference's Python tail yields
 * (feos_torch/pcsaft_pure.py:196-199 / :212-215 / :228-233).
 *   which    0 = vapor_pressure, 1 = liquid_density, 2 = equilibrium_liquid_density; 0 | PCS_JAC_POLISH: rho_vl comes
 *            from pcs_pure_vapor_pressure (~1e-9 from the root) and takes one fp64 Newton step before the derivatives;
 *            3 = boiling_temperature: temp [n] and rho_vl [n,2] are the outputs of pcs_pure_boiling_temperature (converged:
 *            no PCS_JAC_POLISH), pressure may be NULL.  With g0 the which = 0 Jacobian at that state (implicit-function
 *            theorem on p_sat(parameters, T) = p):  jac[k] = -g0[k] / g0[8] (k < 8),  jac[8] = 0,  jac[9] = 1 / g0[8]
 *   pressure [n]    in  Pa (which = 1 only, else NULL)
 *   rho_vl   [n,2]  in  A^-3 (rho_V, rho_L) from pcs_pure_vle; for which = 1 column 1 holds
 *                       rho_root from pcs_pure_liquid_density, column 0 is ignored
 *   jac      [n,10] out d value / d (m, sigma, epsilon_k, mu, kappa_ab, epsilon_k_ab, na, nb, T, p)
 */
#define PCS_JAC_POLISH 0x100
int pcs_pure_jacobian(int which, const double* params, const double* temp, const double* pressure,
                      const double* rho_vl, int64_t n, double* jac, void* stream);

/*
 * The same Jacobian in vector-Jacobian form -- the backward pass of a property call: grad_x[i] = gout[i] * d value_i / d x_i
 * written straight into the dense gradient arrays (no [n,10] round trip through memory).
 *   gout [n] in; grad_params [n,8] (16-byte aligned), grad_temp [n], grad_pressure [n] out, each optional.
 *   which = 3: grad_params and grad_pressure; grad_temp, if given, is zeroed (the temperature is the property, not an input).
 */
int pcs_pure_jacobian_vjp(int which, const double* params, const double* temp, const double* pressure, const double* rho_vl,
                          const double* gout, int64_t n, double* grad_params, double* grad_temp, double* grad_pressure,
                          void* stream);

/*
 * Vapour-liquid critical point of every parameter row: the state (T_c, rho_c) with
 *     p_rho / kT = 1 + rho a'' = 0,   p_rhorho / kT = a'' + rho a''' = 0,   p_rhorhorho > 0
 * (a: reduced residual Helmholtz energy density, p / kT = rho - a + rho a') and p_c = p(T_c, rho_c).  Where the equation of
 * state has more than one such point (strongly polar rows: a second loop at liquid-like densities, at low temperatures), the
 * one with the highest temperature is returned -- the end of the vapour-liquid region: above it the isotherms are
 * mechanically stable at every density, below it pcs_pure_vle finds an equilibrium.  The reference has no counterpart (the
 * engine it wraps offers a critical-point solve that its Python layer does not expose).
 *   params  [n,8]  in   (16-byte aligned)
 *   t_init  [n]    in   K, optional: temperature the bracketing of T_c starts from instead of 0.95 * 1.28 eps m^0.45
 *   tc      [n]    out  K        (optional)
 *   pc      [n]    out  Pa       (optional)
 *   rhoc    [n]    out  kmol/m3  (optional)
 *   status  [n]    out  uint8, 1 = failed (non-finite / non-physical parameters, iteration cap, iterate outside
 *                       T > 0, 0 < eta < 0.7, or p_rhorhorho <= 0 at the converged point); outputs of such rows are 0
 *   iters   [n]    out  int32 Newton iterations, -1 for failed rows (optional, diagnostics)
 * One kernel, no workspace.
 */
int pcs_pure_critical_point(const double* params, const double* t_init, int64_t n, double* tc, double* pc, double* rhoc,
                            uint8_t* status, int32_t* iters, void* stream);

/*
 * Backward pass of pcs_pure_critical_point at converged rows, by the implicit-function theorem
 * (d(T_c, rho_c)/dtheta = -J^-1 dF/dtheta with F = (p_rho, p_rhorho), dp_c/dtheta = p_theta + p_T dT_c/dtheta):
 *   grad_params[i,k] = g_tc[i] dT_c/dtheta_k + g_pc[i] dp_c/dtheta_k + g_rhoc[i] drho_c/dtheta_k.
 *   tc [n] K, rhoc [n] kmol/m3 in: outputs of pcs_pure_critical_point (rows with status 1 give NaN rows: mask them);
 *   g_tc, g_pc, g_rhoc [n] in, each optional (NULL = zero cotangent); grad_params [n,8] out (16-byte aligned).
 */
int pcs_pure_critical_point_vjp(const double* params, const double* tc, const double* rhoc, int64_t n, const double* g_tc,
                                const double* g_pc, const double* g_rhoc, double* grad_params, void* stream);

/*
 * Boiling (saturation) temperature of every parameter row at a given pressure: the T with p_sat(T) = pressure, the inverse of
 * pcs_pure_vle / pcs_pure_vapor_pressure, with the saturated densities at that T.  Safeguarded Newton in (1/T, ln p) on fp64
 * VLE solves, bracketed from above by the critical point (csrc/pure_boiling.hpp).  The reference has no counterpart.
 *   params   [n,8]  in   (16-byte aligned)
 *   pressure [n]    in   Pa
 *   t_init   [n]    in   K, optional: first iterate instead of the corresponding-states estimate from (T_c, p_c)
 *   temp     [n]    out  K     (optional)
 *   rho_vl   [n,2]  out  A^-3: (rho_V, rho_L) at the returned temperature (optional)
 *   status   [n]    out  uint8, 1 = failed: non-finite / non-physical parameters, a pressure that is non-finite, <= 0 or
 *                        >= p_c, a non-finite or non-positive t_init, the iteration cap, or a pressure so close to p_c that
 *                        no VLE solve succeeds inside the closed bracket; outputs of such rows are 0
 *   iters    [n]    out  int32 trial temperatures used, -1 for failed rows (optional, diagnostics)
 * One kernel, no workspace.  Backward pass: pcs_pure_jacobian / pcs_pure_jacobian_vjp with which = 3.
 */
int pcs_pure_boiling_temperature(const double* params, const double* pressure, const double* t_init, int64_t n, double* temp,
                                 double* rho_vl, uint8_t* status, int32_t* iters, void* stream);

/*
 * Enthalpy of vaporization of every parameter row at a given temperature, with the saturated densities at that T:
 *   dh_vap = T (v_V - v_L) dp_sat/dT = R T [s(rho_L) - s(rho_V)],  s = T d(a/rho)/dT + a/rho + ln rho   (csrc/pure_enthalpy.hpp),
 * on an all-fp64 VLE solve whose densities are converged to rounding (dh_vap is first order in their error).  The reference
 * has no counterpart.
 *   params   [n,8]  in   (16-byte aligned)
 *   temp     [n]    in   K
 *   dh       [n]    out  kJ/mol  (optional)
 *   rho_vl   [n,2]  out  A^-3: (rho_V, rho_L) at temp (optional)
 *   status   [n]    out  uint8, 1 = failed: non-finite / non-physical parameters, a temperature that is non-finite or <= 0,
 *                        no vapour-liquid equilibrium (every T >= T_c), or a result that is non-finite or <= 0; outputs of
 *                        such rows are 0
 * One kernel, no workspace.
 */
int pcs_pure_enthalpy_of_vaporization(const double* params, const double* temp, int64_t n, double* dh, double* rho_vl,
                                      uint8_t* status, void* stream);

/*
 * Backward pass of pcs_pure_enthalpy_of_vaporization on solved rows: the TOTAL derivative of dh_vap along the saturation line
 * (the densities respond to the parameters and the temperature; implicit-function theorem on equal pressure and chemical
 * potential in adjoint form, csrc/pure_enthalpy.hpp), times the cotangent.
 *   params   [n,8]  in   (16-byte aligned)
 *   temp     [n]    in   K
 *   rho_vl   [n,2]  in   A^-3, the densities the forward call returned
 *   g_dh     [n]    in   cotangent of dh [kJ/mol]
 *   g_params [n,8]  out  g_dh * d dh / d parameters  (optional, 16-byte aligned)
 *   g_temp   [n]    out  g_dh * d dh / dT [kJ/mol/K] (optional)
 * Rows that are not a converged equilibrium (rho_vl = 0 of a failed row) give non-finite numbers: mask by status.
 */
int pcs_pure_enthalpy_of_vaporization_vjp(const double* params, const double* temp, const double* rho_vl, int64_t n,
                                          const double* g_dh, double* g_params, double* g_temp, void* stream);

/*
 * Binary-mixture bubble point (dew = 0: z = liquid mole fraction of component 1) or dew point
 * (dew = 1: z = vapour mole fraction of component 1) at fixed temperature.
 * Replaces PcSaft.bubble_point / PcSaft.dew_point(parameters[N,2,8], kij[N,2], temperature[N],
 * molefracs[N], pressure[N]) -> (rho[n_ok,4], status[N])  (src/pcsaft.rs:43-79, :150-231) and
 * the Python tails PcSaftMix.bubble_point / dew_point (feos_torch/pcsaft_mix.py:422-468).
 *   params  [n,2,8] in    component rows as for the pure model
 *   kij     [n,2]   in    kij[:,0] = k_ij, kij[:,1] = explicit eps_AiBj/k, 0 = combining rule
 *                         (src/pcsaft.rs:163, pcsaft_mix.py:509-516)
 *   temp, z, p_init [n] in    K, -, Pa (p_init = the caller's starting pressure, src/pcsaft.rs:174); 0 < z < 1: a row at
 *                         z = 0 or z = 1 (a pure component, no mixture) fails; a trace amount down to the smallest
 *                         subnormal either converges to the limit of the dilute solution or fails
 *   p_out   [n]     out   Pa   pcsaft_mix.py:443-444 / :467-468                 (optional)
 *   rho4    [n,4]   out   A^-3 (rhoV_1, rhoV_2, rhoL_1, rhoL_2), src/pcsaft.rs:225-228 (optional)
 *   status  [n]     out   uint8, 1 = failed
 *   iters   [n]     out   int32 Newton iterations (optional)
 *   workspace       device scratch of pcs_mix_workspace_bytes(n) for the work-queue schedule (rows ordered by
 *                   class on the device, a pre-pass with the pure-component fugacities of Raoult's law, persistent
 *                   waves, a lane that finishes a row takes the next one);
 *                   NULL = one row per lane in a single pass (same results, several times slower)
 */
int64_t pcs_mix_workspace_bytes(int64_t n);
int pcs_mix_bubble_dew(int dew, const double* params, const double* kij, const double* temp, const double* z,
                       const double* p_init, int64_t n, double* p_out, double* rho4, uint8_t* status, int32_t* iters,
                       void* workspace, void* stream);

/*
 * Binary-mixture bubble (dew = 0) / dew (dew = 1) TEMPERATURE at a given pressure: the T with p_bubble(T, z) = p_spec
 * (resp. p_dew), the inverse of pcs_mix_bubble_dew in its temperature argument, with the partial densities of both phases at
 * that T.  Safeguarded Newton on f = ln p(T) - ln p_spec in 1/T inside one kernel (csrc/mix_temperature.hpp): every trial is
 * the bubble / dew solve of pcs_mix_bubble_dew at the trial temperature with the initial pressure p_spec -- cold at the first
 * iterate, from the densities of the last solved trial afterwards --, p(T) is that solve's pressure, and the slope
 * d ln p / dT is a temperature tangent at fixed densities.  The reference has no counterpart.
 *   params  [n,2,8] in   (16-byte aligned)
 *   kij     [n,2]   in   (16-byte aligned) as for pcs_mix_bubble_dew
 *   p_spec  [n]     in   Pa, the specified pressure
 *   z       [n]     in   mole fraction of component 1 in the specified phase (liquid for bubble, vapour for dew), 0 < z < 1
 *   t_init  [n]     in   K, the first iterate (mandatory, as the initial pressure of pcs_mix_bubble_dew is)
 *   t_out   [n]     out  K     (optional)
 *   rho4    [n,4]   out  A^-3 (rhoV_1, rhoV_2, rhoL_1, rhoL_2) at t_out: what pcs_mix_jacobian needs (optional, 16-byte aligned)
 *   status  [n]     out  uint8, 1 = failed; outputs of such rows are 0.  A row fails AT ONCE when p_spec or t_init is
 *                        non-finite or <= 0, z is non-finite or outside 0 < z < 1, or a parameter or kij entry is non-finite;
 *                        otherwise when: no trial finds an equilibrium at t_init nor at 8 temperatures below it (each lower
 *                        by a factor 1.1); p_spec lies above the highest pressure of the line (the bracket between a solved
 *                        trial and one without an equilibrium closes to 1e-6); a solved trial has a slope d ln p / dT that is
 *                        not positive and finite -- the retrograde dew branch near a mixture critical point, where the
 *                        pressure falls with the temperature, is not served --; or after 40 trials.
 *                        Accepted: |ln p(T) - ln p_spec| <= 1e-12, or <= 1e-11 directly after a trial within 1e-8 (rounding
 *                        floor of the inner solve); d ln p / d ln T > 1 on these lines, so T is at least as good.
 *   iters   [n]     out  int32 trial temperatures used, -1 for failed rows (optional, diagnostics)
 *   workspace            optional device scratch of pcs_workspace_bytes(n): the rows are then taken in batch-wide class
 *                        order (class-uniform waves); results are identical.  One row per lane, no work queue.
 * A row's result does not depend on the rows it shares a wave with.  Backward pass: J = pcs_mix_jacobian at (t_out, rho4);
 * implicit-function theorem on p(theta, T) = p_spec:  dT/dtheta = -J[:, :18] / J[:, 18],  dT/dp_spec = 1 / J[:, 18].
 */
int pcs_mix_bubble_dew_temperature(int dew, const double* params, const double* kij, const double* p_spec, const double* z,
                                   const double* t_init, int64_t n, double* t_out, double* rho4, uint8_t* status,
                                   int32_t* iters, void* workspace, void* stream);

/*
 * Density of a binary mixture at given (T, p, x): the liquid-like (phase = 0) or the vapour-like (phase = 1) root of
 * p(x rho, (1 - x) rho) = p_spec along the composition line, one kernel (csrc/mix_density.hpp), ABI 114.  Reduced units as for
 * pcs_mix_derivatives; with a, a', a'' the Helmholtz energy density and its derivatives along the line rho_i = x_i rho,
 *     p(rho) = rho - a + rho a',    dp/drho = 1 + rho a'',    p_spec = p [Pa] 1e-30 / (k_B T),    eta = packing(x) rho.
 * The roots:
 *   liquid, with rho_s = 0.5 / packing:
 *     p(rho_s) >= p_spec: the largest rho <= rho_s with p(rho) = p_spec, provided dp/drho > 0 on all of [rho, rho_s]; if
 *                         dp/drho reaches 0 first, the liquid branch ends above p_spec and the row fails;
 *     p(rho_s) <  p_spec: the smallest rho > rho_s with p(rho) = p_spec, dp/drho > 0 and eta < 0.74; if there is none, the row
 *                         fails.
 *     This is the root the bubble-point initialisation takes (start at eta = 0.5, scaled Newton, first bracket above
 *     eta = 0.5), converged to rounding.
 *   vapour: the smallest rho > 0 with p(rho) = p_spec, provided dp/drho > 0 on (0, rho]; started at the ideal gas
 *           rho = p_spec (at eta = 0.05 where the ideal gas is denser: far above the branch it lies at liquid densities); the
 *           row fails if the branch ends first.
 * Safeguarded Newton inside a bracket kept on the branch, bisection where a step leaves the bracket or dp/drho <= 0; the
 * branch is walked from its start in steps of at most a factor 0.8 (down) / 1.25 (up) in density, 0.06 in eta above
 * eta = 0.5, so that a step cannot reach the other branch.  Accepted: |d rho| <= 1e-14 rho, or a step that has stopped
 * shrinking below 1e-12 rho (rounding floor); at most 64 evaluations per row.
 *   params   [n,2,8] in   (16-byte aligned)
 *   kij      [n,2]   in   (16-byte aligned) as for pcs_mix_bubble_dew
 *   temp     [n]     in   K
 *   pressure [n]     in   Pa
 *   x        [n]     in   mole fraction of component 1, 0 <= x <= 1 (both ends are valid)
 *   rho      [n]     out  A^-3, the total density                                     (optional)
 *   dpdrho   [n]     out  the reduced dp/drho along x at the root (> 0)                (optional)
 *   status   [n]     out  uint8, 1 = failed; outputs of such rows are 0.  A row fails AT ONCE when T, p or x is non-finite,
 *                         T <= 0, p <= 0 or x outside [0, 1]; otherwise by the root definitions above, where an evaluation is
 *                         not finite, or at the cap
 *   iters    [n]     out  int32 evaluations used, -1 for failed rows (optional)
 *   workspace             optional, pcs_workspace_bytes(n): the batch-wide class order of pcs_mix_derivatives_vjp.  Accepted
 *                         and NOT used: the rows are taken in their own order (one row per lane, no work queue, no LDS)
 * A row's result does not depend on the rows it shares a wave with.  Backward pass: G = pcs_mix_derivatives_vjp at
 * (x rho, (1 - x) rho) with g_p = -g / dpdrho and no other weight:  d rho/d(params, kij) = G[:, :18],
 * d rho/dT = G[:, 18] + g_p p_spec / T,  d rho/dp [Pa] = -g_p 1e-30 / (k_B T),  d rho/dx = rho (G[:, 19] - G[:, 20]).
 */
int pcs_mix_density(int phase, const double* params, const double* kij, const double* temp, const double* pressure,
                    const double* x, int64_t n, double* rho, double* dpdrho, uint8_t* status, int32_t* iters,
                    void* workspace, void* stream);

/*
 * Henry's law constant of a solute at infinite dilution in a pure, saturated solvent (ABI 117), one kernel
 * (csrc/mix_henry.hpp).  With s the solute (component index `solute`), v the other component (the solvent), rho_L the
 * saturated liquid density of the PURE solvent at T and mu_s = da/drho_s the residual chemical potential of the binary
 * model at the partial densities rho_v = rho_L, rho_s = 0 (the mu of pcs_mix_derivatives there):
 *     H = lim_{x_s -> 0} f_s / x_s = rho_L k_B T exp(mu_s) = rho_L [A^-3] T (k_B / A^3) exp(mu_s)        [Pa]
 * the fugacity-based (IUPAC) constant.  The K-factor form y p / x differs from it by the solute's vapour-phase fugacity
 * coefficient and is not computed; rho_vl and p_sat are handed out for a caller who composes it with pcs_mix_derivatives.
 * The solvent's saturated state is that of pcs_pure_enthalpy_of_vaporization (the all-fp64 VLE solve, densities polished by
 * exact coupled Newton updates until the relative step is below 1e-10, at most three): H is not stationary in the density.
 * The reference has no counterpart.
 *   solute                0 or 1: the component at infinite dilution; anything else is an error return
 *   params    [n,2,8] in   (16-byte aligned)
 *   kij       [n,2]   in   (16-byte aligned) as for pcs_mix_bubble_dew
 *   temp      [n]     in   K
 *   h         [n]     out  Pa
 *   rho_vl    [n,2]   out  A^-3, (rho_V, rho_L) of the pure solvent at T                              (optional)
 *   p_sat     [n]     out  Pa, the pure solvent's vapour pressure (equal-area pressure at rho_vl)      (optional)
 *   dlnh_drho [n]     out  A^3, d ln H / d rho_L = 1 / rho_L + d mu_s / d rho_v at (rho_L, 0)          (optional)
 *   status    [n]     out  uint8, 0 = solved, 1 = failed; outputs of a failed row are 0.  A row fails when a parameter of
 *                          EITHER component is non-finite or m, sigma, eps <= 0 or kappa, eps_ab, na, nb < 0, kij is
 *                          non-finite, T is non-finite or <= 0, the solvent has no equilibrium at T (every T >= T_c of the
 *                          solvent), or H is non-finite or <= 0.  A supercritical solute is an ordinary row.
 * A row's result does not depend on the rows it shares a wave with.  Backward pass, no kernel of its own, with upstream g
 * on H: G = pcs_mix_derivatives_vjp at (rho_L, 0) with g_mu = g H on the solute's column and no other weight gives the
 * explicit part G[:, :19]; the response of rho_L is pcs_pure_jacobian_vjp (selector 2, value in kmol/m3) on the solvent's
 * parameter row with gout = g H dlnh_drho x (1e3 N_A 1e-30), added to the solvent's 8 columns and to T; and g H / T.
 */
int pcs_mix_henry(int solute, const double* params, const double* kij, const double* temp, int64_t n, double* h,
                  double* rho_vl, double* p_sat, double* dlnh_drho, uint8_t* status, void* stream);

/*
 * PcSaftMix.derivatives (feos_torch/pcsaft_mix.py:395-420) at given partial densities rho [n,2]:
 * a [n], p [n] (reduced), residual chemical potentials mu [n,2], partial molar volumes v [n,2].
 * Any output may be NULL.
 */
int pcs_mix_derivatives(const double* params, const double* kij, const double* temp, const double* rho, int64_t n,
                        double* a, double* p, double* mu, double* v, void* stream);

/*
 * Tangent-plane stability analysis of binary feed states (PcSaftMix.stability_analysis).  Reduced units as for
 * pcs_mix_derivatives: a(rho_1, rho_2) = residual Helmholtz energy density / kT [A^-3], mu_i = ln rho_i + da/drho_i,
 * p = sum rho_k - a + sum rho_k da/drho_k.
 *   Feed: T and partial densities rho^f -> p^f, z_i = rho^f_i / sum rho^f.
 *   Trial phase: partial densities rho^t at the same T with p(rho^t) = p^f on a mechanically stable root (dp/drho > 0 along
 *   its composition w_i = rho^t_i / sum rho^t);  tpd(rho^t) = sum_i w_i (mu_i(rho^t) - mu_i(rho^f))  [kT per mole of trial
 *   phase] = Michelsen's sum_i w_i (ln w_i + ln phi_i(w) - ln z_i - ln phi_i(z)).  A trial with |w_1 - z_1| < 1e-6 and
 *   |sum rho^t / sum rho^f - 1| < 1e-6 is trivial and never counts.  TPD_TOL = 1e-8.
 *   params [n,2,8], kij [n,2], temp [n], rho [n,2]   in   (rho: the feed's partial densities, A^-3)
 *   tpd       [n]     out  (optional) smallest tpd among the non-trivial stationary points the search reached; +inf when it
 *                          reached none, -inf for status 2, NaN for status 3
 *   rho_trial [n,2]   out  (optional) partial densities of the trial phase of `tpd` (NaN when there is none)
 *   status    [n]     out  uint8: 0 stable (no trial with tpd < -TPD_TOL), 1 unstable (one found), 2 locally unstable feed
 *                          (the Hessian of a + sum rho_i (ln rho_i - 1) in rho is not positive definite; no search),
 *                          3 invalid feed (non-finite or non-positive density, or p^f <= 0)
 * Search: Michelsen's successive substitution in ln(w_1 / w_2) with Newton steps where tpd is locally convex, from four
 * fixed starts (ideal gas at the feed's chemical potentials on the vapour-like root; liquid-like roots rich in either
 * component, and equimolar).  On a converged bubble / dew point the incipient phase is such a stationary point (tpd ~ 0).  Rows of
 * pcs_mix_bubble_dew that converged through the stagnation exit (|d mu| up to 1e-3) may come out unstable: their
 * incipient phase does not have equal chemical potentials.
 */
int pcs_mix_stability(const double* params, const double* kij, const double* temp, const double* rho, int64_t n,
                      double* tpd, double* rho_trial, uint8_t* status, void* stream);

/*
 * n-component mixtures: PcSaftMix.derivatives for parameters [n, ncomp, 8] WITHOUT k_ij -- the parts of the
 * reference's model that are written for any number of components (feos_torch/pcsaft_mix.py:31-154: hard sphere, hard chain,
 * dispersion, dipoles, self association of ONE associating component; "kij can only be used for binary mixtures", :75-76, and two
 * associating components are binary-only, :250 / :336 -- both stay with pcs_mix_derivatives).
 *   params [n,ncomp,8], temp [n], rho [n,ncomp] in;  a [n], p [n], mu [n,ncomp], v [n,ncomp] out (each optional); 1 <= ncomp <= 6.
 * A row with more than one associating component gets NaN in every output (the reference raises).
 */
int pcs_mixn_derivatives(const double* params, const double* temp, const double* rho, int ncomp, int64_t n, double* a, double* p,
                         double* mu, double* v, void* stream);

/*
 * Backward pass of pcs_mixn_derivatives -- the reference's n-component model is an ordinary torch graph
 * (feos_torch/pcsaft_mix.py:31-154, :395-420), so its autograd reaches parameters, temperature and densities:
 *   grad [n, 9 ncomp + 1] = d L / d (params [ncomp][8], T, rho [ncomp]),  L = g_a a + g_p p + g_mu . mu + g_v . v
 * with the upstream gradients g_a [n], g_p [n], g_mu [n,ncomp], g_v [n,ncomp] (each optional, NULL = 0).  One forward-mode
 * pass per input direction through the same model code (correct first, not tuned: 9 ncomp + 1 evaluations per row).
 */
int pcs_mixn_derivatives_vjp(const double* params, const double* temp, const double* rho, int ncomp, int64_t n, const double* g_a,
                             const double* g_p, const double* g_mu, const double* g_v, double* grad, void* stream);

/*
 * Gradient of the bubble (dew = 0) / dew (dew = 1) pressure [Pa] at the converged densities rho4
 * (from pcs_mix_bubble_dew) — what torch reverse mode through feos_torch/pcsaft_mix.py:435-444 /
 * :459-468 yields.  jac [n,19] = d p / d (params[0,0..7], params[1,0..7], kij[0], kij[1], T).
 * workspace: device scratch of pcs_workspace_bytes(n) or NULL.  With it the rows are processed in batch-wide class
 * order (waves of non-polar / non-associating rows skip the structurally-zero directions); results are identical.
 */
int pcs_mix_jacobian(int dew, const double* params, const double* kij, const double* temp, const double* rho4,
                     int64_t n, double* jac, void* workspace, void* stream);

/*
 * Gradients of TWO functionals of a converged bubble (dew = 0) / dew (dew = 1) point in one kernel (ABI 111): the pressure,
 * as pcs_mix_jacobian, and the composition of the INCIPIENT phase.  Inputs as pcs_mix_jacobian: (temp, rho4) are the state
 * pcs_mix_bubble_dew or pcs_mix_bubble_dew_temperature returned.
 *   jac_p [n,19]  out  d p / d (params[0,0..7], params[1,0..7], kij[0], kij[1], T), Pa per unit (optional)
 *   jac_y [n,19]  out  d y / d (the same 19), y = the mole fraction of COMPONENT 1 in the incipient phase -- the vapour for
 *                      bubble, y = rhoV_1 / (rhoV_1 + rhoV_2), the liquid for dew, y = rhoL_1 / (rhoL_1 + rhoL_2) -- at fixed
 *                      composition of the specified phase (optional)
 * Either output may be NULL, not both (error).  y has no explicit dependence on the inputs: with u = (ln rho_spec,
 * ln rho_inc_1, ln rho_inc_2) and F = (mu_1^S - mu_1^I, mu_2^S - mu_2^I, p^S - p^I) = 0,  dy/dtheta = -w . dF/dtheta|_u with
 * J^T w = dy/du = (0, y (1 - y), -y (1 - y)); the coefficient set, both phase evaluations and the elimination of J^T are
 * shared with the pressure gradient (csrc/mix_incipient.hpp).  A row whose 3x3 system is singular gets NaN in its outputs;
 * rows with rho4 = 0 (failed rows of the solve) get unspecified values and do not disturb the others.
 * workspace: device scratch of pcs_workspace_bytes(n) or NULL, as pcs_mix_jacobian (batch-wide class order; results are
 * identical).  A row's result does not depend on its wave mates, on n, on the workspace or on which outputs are requested.
 * Along a line of constant pressure (backward pass of pcs_mix_bubble_dew_temperature with the composition), from the two
 * blocks at (t_out, rho4), by the implicit-function theorem on p(theta, T) = p_spec:
 *   dT/dtheta = -jac_p[:, :18] / jac_p[:, 18],                          dT/dp_spec = 1 / jac_p[:, 18]
 *   dy/dtheta|_p = jac_y[:, :18] - jac_y[:, 18] jac_p[:, :18] / jac_p[:, 18],   dy/dp_spec = jac_y[:, 18] / jac_p[:, 18]
 */
int pcs_mix_point_jacobian(int dew, const double* params, const double* kij, const double* temp, const double* rho4,
                           int64_t n, double* jac_p, double* jac_y, void* workspace, void* stream);

/*
 * ---- heterosegmented gc-PC-SAFT (binary mixtures) -----------------------------------------
 * Replaces the reference's stateful GcPcSaft class (src/gc_pcsaft.rs:15-99: segment records,
 * per-row chemical records, binary segment records, phi) and the Python tails of
 * GcPcSaftMix.bubble_point / dew_point (feos_torch/gc_pcsaft.py:470-512).
 *
 *   table  [S*8 + 3*S*S] in   per-batch: seg[S][8] (m, sigma, epsilon_k, mu, kappa_ab, epsilon_k_ab,
 *                             na, nb), E1[S][S] = sqrt(eps_a eps_b) sigma_ab^3, E2[S][S] = eps_a eps_b
 *                             sigma_ab^3, K[S][S] = 1 - k_ab, sigma_ab = (sigma_a + sigma_b)/2; S <= 32
 *   rows   [n,80] uint8  in   (16-byte aligned: the kernels take a row with five 16-byte loads)
 *                             molecule structures: for each of the 2 molecules up to 8 entries of
 *                             seg_id [0:16], seg_cnt [16:32], bond_a [32:48], bond_b [48:64],
 *                             bond_cnt [64:80] (count 0 = unused entry)
 *   phi    [n,2]         in   src/gc_pcsaft.rs:30, feos_torch/gc_pcsaft.py:182-185
 *   temp, z, p_init [n]  in   as for pcs_mix_bubble_dew, 0 < z < 1 included (the same solver: z = 0 or 1 fails, a trace
 *                             amount either converges to the limit of the dilute solution or fails)
 *   outputs, workspace        as for pcs_mix_bubble_dew
 *   order  [n] int32     in   optional (NULL: rows are bucketed by class inside each workgroup): a permutation of the rows,
 *                             position -> row, normally sorted by model class (association class x polarity) so that a
 *                             wavefront runs one set of branches.  The rows of a model are fixed, so the caller computes
 *                             it once.  Only the schedule changes: results are identical.
 */
int64_t pcs_gc_table_doubles(int S);
int pcs_gc_bubble_dew(int dew, const double* table, int S, const uint8_t* rows, const double* phi, const double* temp,
                      const double* z, const double* p_init, int64_t n, double* p_out, double* rho4, uint8_t* status,
                      int32_t* iters, const int32_t* order, void* workspace, void* stream);

/*
 * gc-PC-SAFT bubble (dew = 0) / dew (dew = 1) TEMPERATURE at a given pressure (ABI 112): the T with p_bubble(T, z) = p_spec
 * (resp. p_dew), the inverse of pcs_gc_bubble_dew in its temperature argument, with the partial densities of both phases at
 * that T.  The outer iteration is that of pcs_mix_bubble_dew_temperature (csrc/mix_temperature.hpp, one code for both):
 * safeguarded Newton on f = ln p(T) - ln p_spec in 1/T, slope from a temperature tangent at fixed densities, trials
 * warm-started from the last solved one, an accepted warm trial confirmed by a cold one.  A cold trial is the solve of
 * pcs_gc_bubble_dew without a work list at the trial temperature with the initial pressure p_spec (csrc/gc_temperature.hpp),
 * so pcs_gc_bubble_dew at t_out answers p_spec.  The reference has no counterpart.
 *   table, S, rows, phi  in   as for pcs_gc_bubble_dew (rows 16-byte aligned)
 *   p_spec  [n]     in   Pa, the specified pressure
 *   z       [n]     in   mole fraction of component 1 in the specified phase (liquid for bubble, vapour for dew), 0 < z < 1
 *   t_init  [n]     in   K, the first iterate (mandatory)
 *   t_out   [n]     out  K     (optional)
 *   rho4    [n,4]   out  A^-3 (rhoV_1, rhoV_2, rhoL_1, rhoL_2) at t_out: what pcs_gc_jacobian and pcs_gc_segment_gradient
 *                        need (optional, 16-byte aligned)
 *   status  [n]     out  uint8, 0 = solved, 1 = failed; a failed row has t_out = 0, rho4 = 0, iters = -1.  A row fails AT ONCE
 *                        when p_spec or t_init is non-finite or <= 0, z is non-finite or outside 0 < z < 1, or phi is
 *                        non-finite; otherwise when: no trial finds an equilibrium at t_init nor at 8 temperatures below it
 *                        (each lower by a factor 1.1); p_spec lies above the highest pressure of the line (the bracket between
 *                        a solved trial and one without an equilibrium closes to 1e-6); a solved trial has a slope
 *                        d ln p / dT that is not positive and finite -- the retrograde dew branch near a mixture critical
 *                        point is not served --; or after 40 trials.
 *                        Accepted: |ln p(T) - ln p_spec| <= 1e-12, or <= 1e-11 directly after a trial within 1e-8.
 *   iters   [n]     out  int32 trial temperatures used, -1 for failed rows (optional, diagnostics)
 *   order   [n]     in   optional class order of the rows as for pcs_gc_bubble_dew (NULL: bucketed by class inside each
 *                        workgroup); only the schedule changes, results are identical.  One row per lane, no work queue.
 * A row's result does not depend on the rows it shares a wave with.  Backward pass: J = pcs_gc_jacobian at (t_out, rho4),
 * implicit-function theorem on p(theta, T) = p_spec: every gradient of the pressure times -1 / J[:, 6], dT/dp_spec = 1 / J[:, 6]
 * (pcs_gc_segment_gradient with gout = -g / J[:, 6] for the segment table).
 */
int pcs_gc_bubble_dew_temperature(int dew, const double* table, int S, const uint8_t* rows, const double* phi,
                                  const double* p_spec, const double* z, const double* t_init, int64_t n, double* t_out,
                                  double* rho4, uint8_t* status, int32_t* iters, const int32_t* order, void* stream);

/*
 * Density of a gc-PC-SAFT row at given (T, p, x) (ABI 115): pcs_mix_density on the gc model, one kernel
 * (csrc/gc_density.hip on density_root of csrc/mix_density.hpp, one code for both models).  Root definitions (liquid from
 * eta = 0.5, vapour from the ideal gas, a row whose branch ends before it reaches p fails instead of returning the other
 * branch's root), acceptance rule, the cap of 64 evaluations and the reduced units are those of pcs_mix_density, with
 * eta = packing(x) rho, packing = pi/6 sum_i x_i sum_segments n m d^3.  The reference has no counterpart.
 *   phase                 0 = liquid, 1 = vapour; anything else is an error return
 *   table, S, rows, phi   in   as for pcs_gc_bubble_dew (rows 16-byte aligned)
 *   temp     [n]     in   K
 *   pressure [n]     in   Pa
 *   x        [n]     in   mole fraction of component 1, 0 <= x <= 1 (both ends are valid: a pure gc fluid)
 *   rho      [n]     out  A^-3, the total density                                     (optional)
 *   dpdrho   [n]     out  the reduced dp/drho along x at the root (> 0)                (optional)
 *   status   [n]     out  uint8, 1 = failed; outputs of such rows are 0.  A row fails AT ONCE when T, p or x is non-finite,
 *                         T <= 0, p <= 0, x outside [0, 1] or phi is non-finite; otherwise by the root definitions, where an
 *                         evaluation is not finite, or at the cap
 *   iters    [n]     out  int32 evaluations used, -1 for failed rows (optional)
 *   order    [n]     in   optional class order of the rows as for pcs_gc_bubble_dew (NULL: bucketed by class inside each
 *                         workgroup); only the schedule changes, results are identical.  One row per lane, no work queue.
 * A row's result does not depend on the rows it shares a wave with.  Backward pass: pcs_gc_derivatives_vjp at
 * (x rho, (1 - x) rho) with g_p = w = -g / dpdrho and no other weight: grad_seg is the segment-table gradient, jac9[:, :6] feed
 * the k_ab and phi chains of the pressure, and  d rho/dT = jac9[:, 6] + w p_spec / T,  d rho/dp [Pa] = -w 1e-30 / (k_B T),
 * d rho/dx = rho (jac9[:, 7] - jac9[:, 8]).
 */
int pcs_gc_density(int phase, const double* table, int S, const uint8_t* rows, const double* phi, const double* temp,
                   const double* pressure, const double* x, int64_t n, double* rho, double* dpdrho, uint8_t* status,
                   int32_t* iters, const int32_t* order, void* stream);

/*
 * Vapour-liquid equilibrium of ONE molecule of a gc-PC-SAFT row taken as a pure fluid (ABI 118): saturation pressure and
 * saturated densities at given T, one kernel (csrc/gc_saturation.hip on pure_line_vle of csrc/gc_saturation.hpp).  The pure
 * fluid is the composition line x = 1 (component 0) or x = 0 (component 1) of the row's model -- k_ab acts between segments
 * of unlike molecules only, so it does not enter --, evaluated as pcs_gc_density evaluates it: p = rho - a + rho a',
 * dp/drho = 1 + rho a''.  Solve: the algorithm of the pure-component robust pass (csrc/pure_solver.hpp, vle_robust) --
 * zero-pressure liquid from eta = 0.5 with the vapour at the liquid's fugacity, else both spinodals and branch solves at the
 * mean of their pressures; coupled Newton on the equal-area pressure p* = -(f_V - f_L)/(v_V - v_L), f = a/rho + ln rho, with
 * backtracking onto the stable branches -- then further Newton updates until both relative steps are below 1e-10 (at most
 * three) and one closing evaluation at the final densities.  The reference has no counterpart.
 *   component             0 or 1: the molecule of each row that is taken as a pure fluid; anything else is an error return
 *   table, S, rows, phi   in   as for pcs_gc_bubble_dew (rows 16-byte aligned)
 *   temp      [n]    in   K
 *   p_sat     [n]    out  Pa: p* T k_B 1e30 with the second-order corrected p* of the closing step       (optional)
 *   rho_vl    [n,2]  out  (rho_V, rho_L) in A^-3                                                         (optional)
 *   dpdrho_vl [n,2]  out  the reduced dp/drho at the two roots (> 0): what the backward pass of rho_L needs (optional)
 *   status    [n]    out  uint8, 1 = failed; outputs of such rows are 0.  A row fails AT ONCE when T is non-finite or <= 0 or
 *                         phi is non-finite; otherwise where the pure fluid has no vapour-liquid equilibrium at T (every T at
 *                         or above its critical temperature: no van der Waals loop, or a non-positive vapour-spinodal
 *                         pressure), where the iteration does not converge within its caps, or where the converged state is
 *                         not accepted: the trivial solution rho_V = rho_L, a pressure that is not 0 < p* <= 1.0001 rho_V (an
 *                         "equilibrium" between two dense states on a second van der Waals loop), or a mechanically unstable
 *                         state at one of the eight halvings of rho_V (the vapour root must lie on the branch from zero
 *                         density).  A failed row never carries any of these.
 *   iters     [n]    out  int32 model evaluations used, -1 for failed rows (optional, diagnostics)
 *   order     [n]    in   optional class order of the rows as for pcs_gc_bubble_dew (NULL: bucketed by class inside each
 *                         workgroup); only the schedule changes, results are identical.  One row per lane, no work queue.
 * A row's result does not depend on the rows it shares a wave with, on n or on order.  Backward pass: two
 * pcs_gc_derivatives_vjp calls accumulating into one grad_seg, at (rho_V, 0) and (rho_L, 0) (component 1: (0, rho)).  With
 * dv = 1/rho_V - 1/rho_L, w = g T k_B 1e30 for an upstream gradient g of p_sat: g_a = -w / (rho_V dv) on the vapour call,
 * g_a = +w / (rho_L dv) on the liquid call (p* is stationary in both densities); d p_sat/dT = g p_sat / T + sum of jac9[:, 6].
 * For rho_L (p_L(rho_L, theta) = p*(theta)): the same with w = g / dpdrho_L, plus g_p = -g / dpdrho_L on the liquid call.
 */
int pcs_gc_pure_vle(int component, const double* table, int S, const uint8_t* rows, const double* phi, const double* temp,
                    int64_t n, double* p_sat, double* rho_vl, double* dpdrho_vl, uint8_t* status, int32_t* iters,
                    const int32_t* order, void* stream);

/*
 * Henry's law constant of ONE molecule of a gc-PC-SAFT row at infinite dilution in the other, pure and saturated, molecule
 * (ABI 120): pcs_mix_henry on the gc model, one kernel (csrc/gc_henry.hip on csrc/gc_henry.hpp).  With s the solute, v = 1 - s
 * the solvent, rho_L the saturated liquid density of molecule v taken as a pure fluid at T (the solve of pcs_gc_pure_vle,
 * pure_line_vle of csrc/gc_saturation.hpp, unchanged) and mu_s = da/drho_s the residual chemical potential of the row's
 * two-molecule model at the partial densities rho_v = rho_L, rho_s = 0 (what pcs_gc_derivatives returns as mu):
 *     H = rho_L k_B T exp(mu_s) = rho_L [A^-3] T k_B 1e30 exp(mu_s)   [Pa],
 * the fugacity-based constant; the K-factor form y p / x is not computed.  mu_s and d mu_s/d rho_v come from ONE two-variable
 * evaluation at that state (the evaluation of pcs_gc_derivatives).  The reference has no counterpart.
 *   solute                0 or 1: the molecule of each row that is infinitely dilute; anything else is an error return
 *   table, S, rows, phi   in   as for pcs_gc_bubble_dew (rows 16-byte aligned)
 *   temp      [n]    in   K
 *   h         [n]    out  Pa                                                                               (required)
 *   rho_vl    [n,2]  out  (rho_V, rho_L) of the pure solvent in A^-3                                        (optional)
 *   p_sat     [n]    out  Pa, the pure solvent's saturation pressure, as pcs_gc_pure_vle                    (optional)
 *   dlnh_drho [n]    out  A^3: d ln H / d rho_L = 1 / rho_L + d mu_s / d rho_v at fixed T and parameters    (optional)
 *   dpdrho_l  [n]    out  the reduced dp/drho of the pure solvent at the liquid root (> 0)                  (optional)
 *   status    [n]    out  uint8, 1 = failed; outputs of such rows are 0.  A row fails AT ONCE when T is non-finite or <= 0 or
 *                         phi is non-finite; otherwise with every failure of pcs_gc_pure_vle on the solvent (no equilibrium
 *                         at T: every T at or above the solvent's critical temperature), or where H or dlnh_drho is not
 *                         finite or H <= 0.  A supercritical solute is an ordinary row.
 *   iters     [n]    out  int32 model evaluations used (the solvent's plus one), -1 for failed rows (optional, diagnostics)
 *   order     [n]    in   optional class order of the rows as for pcs_gc_bubble_dew (NULL: bucketed by class inside each
 *                         workgroup); only the schedule changes, results are identical.  One row per lane, no work queue.
 * A row's result does not depend on the rows it shares a wave with, on n or on order.  Backward pass: two
 * pcs_gc_derivatives_vjp calls accumulating into one grad_seg, at (rho_V, 0) and (rho_L, 0) on the solvent's column.  With
 * gH = g H for an upstream gradient g of H, dv = 1/rho_V - 1/rho_L and w = gH dlnh_drho / dpdrho_l:  g_a = -w / (rho_V dv) on
 * the vapour call;  g_a = +w / (rho_L dv), g_p = -w and g_mu[:, s] = gH on the liquid call;  d H/dT = gH / T + the summed
 * jac9[:, 6]  (d ln H/d theta = @mu_s/@theta + dlnh_drho d rho_L/d theta, d rho_L/d theta as for pcs_gc_pure_vle).
 */
int pcs_gc_henry(int solute, const double* table, int S, const uint8_t* rows, const double* phi, const double* temp, int64_t n,
                 double* h, double* rho_vl, double* p_sat, double* dlnh_drho, double* dpdrho_l, uint8_t* status, int32_t* iters,
                 const int32_t* order, void* stream);

/* GcPcSaftMix.derivatives (feos_torch/gc_pcsaft.py:443-468): a, p, mu [n,2], v [n,2] at rho [n,2]. */
int pcs_gc_derivatives(const double* table, int S, const uint8_t* rows, const double* phi, const double* temp,
                       const double* rho, int64_t n, double* a, double* p, double* mu, double* v, void* stream);

/* GcPcSaftMix.stability_analysis: pcs_mix_stability for gc rows (table / rows / phi as for pcs_gc_bubble_dew).  order: as
 * for pcs_gc_bubble_dew (optional; only the schedule changes, results are identical). */
int pcs_gc_stability(const double* table, int S, const uint8_t* rows, const double* phi, const double* temp,
                     const double* rho, int64_t n, double* tpd, double* rho_trial, uint8_t* status,
                     const int32_t* order, void* stream);

/*
 * Gradient of the gc bubble / dew pressure [Pa] at the converged densities rho4:
 *   jac [n,7] = d p / d (A00, A01, A11, B00, B01, B11, T), the dispersion aggregates
 *               rho1mix = A00 r0^2 + A01 r0 r1 + A11 r1^2, rho2mix likewise with B
 *               (feos_torch/gc_pcsaft.py:177-194) — k_ab and phi enter the model only through them;
 *   agg [n,6] = the aggregate values (optional);
 *   order [n]   = optional class order of the rows as for pcs_gc_bubble_dew (schedule only).
 * The pressure-only launch of pcs_gc_point_jacobian's kernel (csrc/gc_incipient.hip).
 */
int pcs_gc_jacobian(int dew, const double* table, int S, const uint8_t* rows, const double* phi, const double* temp,
                    const double* rho4, int64_t n, double* jac, double* agg, const int32_t* order, void* stream);

/*
 * Gradient of the gc bubble / dew pressures [Pa] w.r.t. the SEGMENT PARAMETER TABLE, contracted with an upstream
 * gradient over the rows — what torch reverse mode through GcPcSaftMix.bubble_point / dew_point delivers to the eight
 * segment parameter vectors passed to the constructor (feos_torch/gc_pcsaft.py:14-22, :54-86, :470-512):
 *   grad_seg [S,8]  +=  sum_i gout[i] * d p_i / d seg[S,8]      (m, sigma, epsilon_k, mu, kappa_ab, epsilon_k_ab, na, nb)
 *   gout     [n]    in   upstream gradient dL/dp_i (NULL = 1 for every row)
 *   grad_seg [S*8]  inout ACCUMULATED with fp64 atomics: the caller zeroes it (or keeps accumulating over shards)
 *   rho4, order     as for pcs_gc_jacobian (converged densities of the same rows; optional class order)
 * d sqrt(eps_a eps_b) / d eps_a is taken as 0 where eps_a = 0 (the square root is not differentiable there; the
 * reference's autograd returns NaN for every epsilon_k of such a table).
 */
int pcs_gc_segment_gradient(int dew, const double* table, int S, const uint8_t* rows, const double* phi, const double* temp,
                            const double* rho4, int64_t n, const double* gout, double* grad_seg, const int32_t* order,
                            void* stream);

/*
 * Gradients of TWO functionals of a converged gc bubble (dew = 0) / dew (dew = 1) point in one kernel (ABI 113): the pressure,
 * as pcs_gc_jacobian, and the composition of the INCIPIENT phase, as pcs_mix_point_jacobian.  Inputs as pcs_gc_jacobian:
 * (temp, rho4) are the state pcs_gc_bubble_dew or pcs_gc_bubble_dew_temperature returned.  Both entry points launch one kernel
 * template (csrc/gc_incipient.hip); pcs_gc_jacobian is this call with jac_y = NULL.
 *   jac_p [n,7]  out  d p / d (A00, A01, A11, B00, B01, B11, T), Pa per unit: pcs_gc_jacobian's jac, bit for bit, whether or
 *                     not jac_y is requested (tests/golden/gc_jacobian_bits.json pins the bits) (optional)
 *   jac_y [n,7]  out  d y / d (the same 7), y = the mole fraction of COMPONENT 1 in the incipient phase -- the vapour for
 *                     bubble, y = rhoV_1 / (rhoV_1 + rhoV_2), the liquid for dew, y = rhoL_1 / (rhoL_1 + rhoL_2) -- at fixed
 *                     composition of the specified phase (optional)
 *   agg   [n,6]  out  the aggregate values, as pcs_gc_jacobian (optional)
 *   order [n]    in   optional class order of the rows as for pcs_gc_bubble_dew (schedule only)
 * Either of jac_p, jac_y may be NULL, not both (error).  y has no explicit dependence on the inputs: with u = (ln rho_spec,
 * ln rho_inc_1, ln rho_inc_2) and F = (mu_1^S - mu_1^I, mu_2^S - mu_2^I, p^S - p^I) = 0,  dy/dtheta = -w . dF/dtheta|_u with
 * J^T w = dy/du = (0, y (1 - y), -y (1 - y)); the coefficient set, both phase evaluations and the elimination of J^T are
 * shared with the pressure gradient (csrc/gc_incipient.hip).  k_ab and phi enter through the aggregates; the caller chains
 * them from either block exactly as from pcs_gc_jacobian's.  A row whose 3x3 system is singular gets NaN in jac_p and jac_y;
 * rows with rho4 = 0 (failed rows of the solve) get unspecified values and do not disturb the others.  A row's result does not
 * depend on its wave mates, on n, on the order or on which outputs are requested.
 * Along a line of constant pressure (backward pass of pcs_gc_bubble_dew_temperature with the composition), from the two
 * blocks at (t_out, rho4), by the implicit-function theorem on p(theta, T) = p_spec:
 *   dT/dtheta = -jac_p[:, :6] / jac_p[:, 6],                            dT/dp_spec = 1 / jac_p[:, 6]
 *   dy/dtheta|_p = jac_y[:, :6] - jac_y[:, 6] jac_p[:, :6] / jac_p[:, 6],     dy/dp_spec = jac_y[:, 6] / jac_p[:, 6]
 */
int pcs_gc_point_jacobian(int dew, const double* table, int S, const uint8_t* rows, const double* phi, const double* temp,
                          const double* rho4, int64_t n, double* jac_p, double* jac_y, double* agg, const int32_t* order,
                          void* stream);

/*
 * Gradient of both functionals of pcs_gc_point_jacobian w.r.t. the SEGMENT PARAMETER TABLE, contracted with their upstream
 * gradients over the rows (ABI 113):
 *   grad_seg [S,8]  +=  sum_i (gout_p[i] * d p_i / d seg[S,8] + gout_y[i] * d y_i / d seg[S,8])
 *   gout_p   [n]    in   upstream gradient dL/dp_i, per Pa (NULL = 0 for every row)
 *   gout_y   [n]    in   upstream gradient dL/dy_i (NULL = 0 for every row); gout_p and gout_y both NULL is an error
 *   grad_seg, rho4, order and the epsilon_k = 0 convention as for pcs_gc_segment_gradient
 * The functional of a row is linear in its phase constants (alpha, beta) -- specified phase: alpha = w2, beta = -w2 rho^S -
 * (w0, w1); incipient phase: alpha = -w2, beta = w2 rho^I + (w0, w1) for y, pcs_gc_segment_gradient's for p -- so the kernel
 * forms (alpha, beta) = gout_p T P_UNIT (alpha, beta)_p + gout_y (alpha, beta)_y from one elimination with two right-hand
 * sides and runs pcs_gc_segment_gradient's machinery ONCE for both: one pass costs what either functional costs alone.  With
 * gout_y = NULL the result is pcs_gc_segment_gradient's up to rounding (the weights enter before, not after, the chain).
 * Along a line of constant pressure, with J_T = jac_p[:, 6], J_yT = jac_y[:, 6] of pcs_gc_point_jacobian and upstream gradients
 * g_T of the temperature and g_y of y:  gout_p = -(g_T + g_y J_yT) / J_T,  gout_y = g_y;  dL/dp_spec = (g_T + g_y J_yT) / J_T.
 */
int pcs_gc_point_segment_gradient(int dew, const double* table, int S, const uint8_t* rows, const double* phi, const double* temp,
                                  const double* rho4, int64_t n, const double* gout_p, const double* gout_y, double* grad_seg,
                                  const int32_t* order, void* stream);

/*
 * ---- vector-Jacobian products of the state functions -------------------------------------------------------------
 * In the reference helmholtz_energy(_density) and derivatives are ordinary torch graphs (feos_torch/pcsaft_pure.py:106-182,
 * pcsaft_mix.py:31-154 / :395-420, gc_pcsaft.py:116-253 / :443-468): a loss built on their outputs back-propagates to the
 * parameters, the temperature and the densities.  These entry points are that backward pass: upstream gradients of the
 * outputs in (NULL = that output does not enter the loss), gradients of the loss w.r.t. the inputs out.  Forward mode
 * inside (dual-number directions per pass), contracted with the upstream gradients in the kernel.
 */

/* PcSaftPure.derivatives -> (a, p, dp).  g_a, g_p, g_dp [n] in; grad_params [n,8], grad_temp [n], grad_rho [n] out
 * (each optional). */
int pcs_pure_derivatives_vjp(const double* params, const double* temp, const double* rho, int64_t n, const double* g_a,
                             const double* g_p, const double* g_dp, double* grad_params, double* grad_temp, double* grad_rho,
                             void* stream);

/* PcSaftMix.derivatives -> (a, p, mu [n,2], v [n,2]).  g_a, g_p [n], g_mu, g_v [n,2] in;
 * grad [n,21] = dL/d(params[0,0..7], params[1,0..7], kij[0], kij[1], T, rho_0, rho_1) out.
 * workspace: optional device scratch of pcs_workspace_bytes(n) (batch-wide class order, as pcs_mix_jacobian). */
int pcs_mix_derivatives_vjp(const double* params, const double* kij, const double* temp, const double* rho, int64_t n,
                            const double* g_a, const double* g_p, const double* g_mu, const double* g_v, double* grad,
                            void* workspace, void* stream);

/* GcPcSaftMix.derivatives -> (a, p, mu, v).  Upstream gradients as for pcs_mix_derivatives_vjp;
 *   grad_seg [S*8] inout  += sum_i dL_i / d seg[S,8]  (accumulated, caller zeroes; see pcs_gc_segment_gradient)
 *   jac9     [n,9]  out   dL_i / d (A00, A01, A11, B00, B01, B11, T, rho_0, rho_1): k_ab and phi enter through the
 *                         six dispersion aggregates (see pcs_gc_jacobian), the caller chains them
 *   agg      [n,6]  out   the aggregate values (optional) */
int pcs_gc_derivatives_vjp(const double* table, int S, const uint8_t* rows, const double* phi, const double* temp,
                           const double* rho, int64_t n, const double* g_a, const double* g_p, const double* g_mu,
                           const double* g_v, double* grad_seg, double* jac9, double* agg, const int32_t* order, void* stream);

/*
 * Order-preserving stream compaction of dense solver outputs.  The reference drops the rows its solver
 * fails on inside the native call (src/pcsaft.rs:93-101, :216-231: `rho[n_ok, ..]` + `status[N]`) and filters the model
 * with the same mask (feos_torch/pcsaft_pure.py:235-243, pcsaft_mix.py:470-479, gc_pcsaft.py:514-528).
 *   pcs_compact_workspace_bytes(n)  bytes of the plan buffer `cws`
 *   pcs_compact_plan    status [n] (uint8, 0 = keep) -> cws; afterwards ((int32_t*)cws)[0] = number of kept rows (the one
 *                       value a caller has to read back to size its outputs)
 *   pcs_compact_rows    dst[j, 0..width) = src[i_j, 0..width) for the j-th kept row, rows of `width` doubles (1..64);
 *                       index [n_ok] (int32, optional) = i_j.  src / dst may be NULL together (index only).
 *   pcs_expand_rows     inverse, fused with the chain rule of the backward pass: dst[i, c] = g[j] * src[j, col0 + c]
 *                       (c < ncol) for kept rows, 0 for dropped ones; src rows have src_stride doubles; g NULL = 1;
 *                       status NULL = every row kept (j = i, cws unused).
 */
int64_t pcs_compact_workspace_bytes(int64_t n);
int pcs_compact_plan(const uint8_t* status, int64_t n, void* cws, void* stream);
int pcs_compact_rows(const uint8_t* status, int64_t n, const void* cws, const double* src, int width, double* dst,
                     int32_t* index, void* stream);
int pcs_expand_rows(const uint8_t* status, int64_t n, const void* cws, const double* g, const double* src, int src_stride,
                    int col0, int ncol, double* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PCSAFT_HIP_H */
