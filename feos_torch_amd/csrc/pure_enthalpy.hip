// Enthalpies of vaporization of pure-component parameter rows and their gradients along the saturation line (see
// include/pcsaft_hip.h: pcs_pure_enthalpy_of_vaporization, pcs_pure_enthalpy_of_vaporization_vjp; solver and formulas in
// pure_enthalpy.hpp).  Own translation unit, compiled with strict IEEE semantics like pure_boiling.hip and pure_critical.hip:
// the failure detection relies on IEEE comparisons and the unit has no fp32 pre-solve (feos_torch_amd/build.py).
//
// Launch shape as the other pure kernels: one row per lane, 256-thread workgroups, the [n,8] parameter rows of a workgroup
// fetched with 16-byte loads and staged through LDS (stage_lane_row, pure_stage.hpp); T, dh, status and the cotangent are SoA, the densities [n,2].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pcsaft_hip.h"
#include "abi_common.hpp"
#include "pure_enthalpy.hpp"
#include "pure_stage.hpp"

using namespace pcs;
using namespace pcs_abi;

namespace {

constexpr int BLOCK = STAGE_BLOCK;

__global__ __launch_bounds__(BLOCK) void k_pure_enthalpy(const double* __restrict__ params, const double* __restrict__ temp,
                                                         int64_t n, double* __restrict__ dh, double* __restrict__ rho_vl,
                                                         uint8_t* __restrict__ status) {
    const LaneRow row = stage_lane_row(params, n);  // pure_stage.hpp: rows past n repeat row n-1 and are never stored
    const int64_t i = row.i, ii = row.ii;
    EnthalpyResult r;
    const int st = enthalpy_of_vaporization(row.par, temp[ii], r);  // wave-uniform call
    if (!row.live) return;
    const bool ok = st == 0;
    if (dh) dh[i] = ok ? r.dh : 0.0;
    if (rho_vl) {
        rho_vl[2 * i] = ok ? r.rho_v : 0.0;
        rho_vl[2 * i + 1] = ok ? r.rho_l : 0.0;
    }
    status[i] = ok ? 0 : 1;
}

__global__ __launch_bounds__(BLOCK) void k_pure_enthalpy_vjp(const double* __restrict__ params, const double* __restrict__ temp,
                                                             const double* __restrict__ rho_vl, int64_t n,
                                                             const double* __restrict__ g_dh, double* __restrict__ g_params,
                                                             double* __restrict__ g_temp) {
    const LaneRow row = stage_lane_row(params, n);  // pure_stage.hpp: rows past n repeat row n-1 and are never stored
    const int64_t i = row.i, ii = row.ii;
    double g[ENTH_DIRS];
    enthalpy_vjp(row.par, temp[ii], rho_vl[2 * ii], rho_vl[2 * ii + 1], g);
    if (!row.live) return;
    // the derivatives are pinned in registers, so that the cotangent cannot be folded into their last operations (the
    // product with a cotangent must equal gout x the unit-cotangent result bit for bit).  A row that is not a converged
    // equilibrium (rho_vl = 0 from a failed solve) gives NaNs: the caller masks by status
#pragma unroll
    for (int k = 0; k < ENTH_DIRS; k++) asm volatile("" : "+v"(g[k]));
    const double go = g_dh[i];
    if (g_params) {
        double2* dst = reinterpret_cast<double2*>(g_params + 8 * i);
#pragma unroll
        for (int k = 0; k < 4; k++) dst[k] = make_double2(go * g[2 * k], go * g[2 * k + 1]);
    }
    if (g_temp) g_temp[i] = go * g[8];
}

}  // namespace

extern "C" {

int pcs_pure_enthalpy_of_vaporization(const double* params, const double* temp, int64_t n, double* dh, double* rho_vl,
                                      uint8_t* status, void* stream) {
    if (int e = enter(n, params && temp && status, "pcs_pure_enthalpy_of_vaporization: null required pointer"); e != GO_ON) return e;
    if (int e = aligned16("pcs_pure_enthalpy_of_vaporization", "params", params)) return e;
    const unsigned grid = grid_for(n, BLOCK);
    hipLaunchKernelGGL(k_pure_enthalpy, dim3(grid), dim3(BLOCK), 0, as_stream(stream), params, temp, n, dh, rho_vl, status);
    return launched("k_pure_enthalpy launch");
}

int pcs_pure_enthalpy_of_vaporization_vjp(const double* params, const double* temp, const double* rho_vl, int64_t n,
                                          const double* g_dh, double* g_params, double* g_temp, void* stream) {
    if (int e = enter(n, params && temp && rho_vl && g_dh, "pcs_pure_enthalpy_of_vaporization_vjp: null required pointer"); e != GO_ON)
        return e;
    if (int e = aligned16("pcs_pure_enthalpy_of_vaporization_vjp", "params and g_params", params, g_params)) return e;
    const unsigned grid = grid_for(n, BLOCK);
    hipLaunchKernelGGL(k_pure_enthalpy_vjp, dim3(grid), dim3(BLOCK), 0, as_stream(stream), params, temp, rho_vl, n, g_dh, g_params,
                       g_temp);
    return launched("k_pure_enthalpy_vjp launch");
}

}  // extern "C"
