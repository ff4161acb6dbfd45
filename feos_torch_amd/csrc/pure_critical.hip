// Critical points of pure-component parameter rows and their parameter gradients (see include/pcsaft_hip.h:
// pcs_pure_critical_point, pcs_pure_critical_point_vjp; solver and formulas in pure_critical.hpp).  Own translation unit,
// compiled with strict IEEE semantics like pure_robust.hip: the bracketing of the critical temperature and the failure
// detection rely on IEEE comparisons (feos_torch_amd/build.py).
//
// Launch shape as the other pure kernels: one row per lane, 256-thread workgroups, the [n,8] parameter rows of a workgroup
// fetched with 16-byte loads and staged through LDS (stage_lane_row, pure_stage.hpp); T_c, p_c, rho_c, status and the cotangents are SoA.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pcsaft_hip.h"
#include "abi_common.hpp"
#include "pure_critical.hpp"
#include "pure_stage.hpp"

using namespace pcs;
using namespace pcs_abi;

namespace {

constexpr int BLOCK = STAGE_BLOCK;

__global__ __launch_bounds__(BLOCK) void k_pure_critical(const double* __restrict__ params, const double* __restrict__ t_init,
                                                         int64_t n, double* __restrict__ tc, double* __restrict__ pc,
                                                         double* __restrict__ rhoc, uint8_t* __restrict__ status,
                                                         int32_t* __restrict__ iters) {
    const LaneRow row = stage_lane_row(params, n);  // pure_stage.hpp: rows past n repeat row n-1 and are never stored
    const int64_t i = row.i, ii = row.ii;
    CritResult r;
    const int st = critical_point(row.par, t_init ? t_init[ii] : 0.0, t_init != nullptr, r);  // wave-uniform call
    if (!row.live) return;
    const bool ok = st == 0;
    if (tc) tc[i] = ok ? r.T : 0.0;
    if (pc) pc[i] = ok ? r.p * r.T * P_UNIT : 0.0;
    if (rhoc) rhoc[i] = ok ? r.rho * (1.0 / RHO_UNIT) : 0.0;
    if (iters) iters[i] = ok ? r.iters : -1;
    status[i] = ok ? 0 : 1;
}

__global__ __launch_bounds__(BLOCK) void k_pure_critical_vjp(const double* __restrict__ params, const double* __restrict__ tc,
                                                             const double* __restrict__ rhoc, int64_t n,
                                                             const double* __restrict__ g_tc, const double* __restrict__ g_pc,
                                                             const double* __restrict__ g_rhoc,
                                                             double* __restrict__ grad_params) {
    const LaneRow row = stage_lane_row(params, n);  // pure_stage.hpp: rows past n repeat row n-1 and are never stored
    const int64_t i = row.i, ii = row.ii;
    double g[8];
    critical_point_vjp(row.par, tc[ii], rhoc[ii] * RHO_UNIT, g_tc ? g_tc[ii] : 0.0, g_pc ? g_pc[ii] : 0.0,
                       g_rhoc ? g_rhoc[ii] : 0.0, g);
    if (!row.live) return;
    // a row that is not a converged critical point (T_c = rho_c = 0 from a failed solve) gives NaNs: the caller masks by status
    double2* dst = reinterpret_cast<double2*>(grad_params + 8 * i);
#pragma unroll
    for (int k = 0; k < 4; k++) dst[k] = make_double2(g[2 * k], g[2 * k + 1]);
}

}  // namespace

extern "C" {

int pcs_pure_critical_point(const double* params, const double* t_init, int64_t n, double* tc, double* pc, double* rhoc,
                            uint8_t* status, int32_t* iters, void* stream) {
    if (int e = enter(n, params && status, "pcs_pure_critical_point: null required pointer"); e != GO_ON) return e;
    if (int e = aligned16("pcs_pure_critical_point", "params", params)) return e;
    const unsigned grid = grid_for(n, BLOCK);
    hipLaunchKernelGGL(k_pure_critical, dim3(grid), dim3(BLOCK), 0, as_stream(stream), params, t_init, n, tc, pc, rhoc, status,
                       iters);
    return launched("k_pure_critical launch");
}

int pcs_pure_critical_point_vjp(const double* params, const double* tc, const double* rhoc, int64_t n, const double* g_tc,
                                const double* g_pc, const double* g_rhoc, double* grad_params, void* stream) {
    if (int e = enter(n, params && tc && rhoc && grad_params, "pcs_pure_critical_point_vjp: null required pointer"); e != GO_ON) return e;
    if (int e = aligned16("pcs_pure_critical_point_vjp", "params and grad_params", params, grad_params)) return e;
    const unsigned grid = grid_for(n, BLOCK);
    hipLaunchKernelGGL(k_pure_critical_vjp, dim3(grid), dim3(BLOCK), 0, as_stream(stream), params, tc, rhoc, n, g_tc, g_pc,
                       g_rhoc, grad_params);
    return launched("k_pure_critical_vjp launch");
}

}  // extern "C"
