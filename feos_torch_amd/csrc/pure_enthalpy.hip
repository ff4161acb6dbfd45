// Enthalpies of vaporization of pure-component parameter rows and their gradients along the saturation line (see
// include/pcsaft_hip.h: pcs_pure_enthalpy_of_vaporization, pcs_pure_enthalpy_of_vaporization_vjp; solver and formulas in
// pure_enthalpy.hpp).  Own translation unit, compiled with strict IEEE semantics like pure_boiling.hip and pure_critical.hip:
// the failure detection relies on IEEE comparisons and the unit has no fp32 pre-solve (feos_torch_amd/build.py).
//
// Launch shape as the other pure kernels: one row per lane, 256-thread workgroups, the [n,8] parameter rows of a workgroup
// fetched with 16-byte loads and staged through LDS (pure_stage.hpp); T, dh, status and the cotangent are SoA, the densities [n,2].
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
constexpr int ROW_PAD = STAGE_ROW_PAD;

__global__ __launch_bounds__(BLOCK) void k_pure_enthalpy(const double* __restrict__ params, const double* __restrict__ temp,
                                                         int64_t n, double* __restrict__ dh, double* __restrict__ rho_vl,
                                                         uint8_t* __restrict__ status) {
    __shared__ double lds[BLOCK * ROW_PAD];
    const int64_t row0 = (int64_t)blockIdx.x * BLOCK;
    const int64_t i = row0 + threadIdx.x;
    const bool live = i < n;
    stage_rows(params, n, row0, lds);
    double par[8];
#pragma unroll
    for (int k = 0; k < 8; k++) par[k] = lds[threadIdx.x * ROW_PAD + k];
    const int64_t ii = live ? i : n - 1;  // rows past n repeat row n-1 and are never stored
    EnthalpyResult r;
    const int st = enthalpy_of_vaporization(par, temp[ii], r);  // wave-uniform call
    if (!live) return;
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
    __shared__ double lds[BLOCK * ROW_PAD];
    const int64_t row0 = (int64_t)blockIdx.x * BLOCK;
    const int64_t i = row0 + threadIdx.x;
    const bool live = i < n;
    stage_rows(params, n, row0, lds);
    double par[8];
#pragma unroll
    for (int k = 0; k < 8; k++) par[k] = lds[threadIdx.x * ROW_PAD + k];
    const int64_t ii = live ? i : n - 1;
    double g[ENTH_DIRS];
    enthalpy_vjp(par, temp[ii], rho_vl[2 * ii], rho_vl[2 * ii + 1], g);
    if (!live) return;
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
    if ((reinterpret_cast<uintptr_t>(params) & 15) != 0)
        return fail_msg("pcs_pure_enthalpy_of_vaporization: params must be 16-byte aligned");
    const unsigned grid = grid_for(n, BLOCK);
    hipLaunchKernelGGL(k_pure_enthalpy, dim3(grid), dim3(BLOCK), 0, as_stream(stream), params, temp, n, dh, rho_vl, status);
    return launched("k_pure_enthalpy launch");
}

int pcs_pure_enthalpy_of_vaporization_vjp(const double* params, const double* temp, const double* rho_vl, int64_t n,
                                          const double* g_dh, double* g_params, double* g_temp, void* stream) {
    if (int e = enter(n, params && temp && rho_vl && g_dh, "pcs_pure_enthalpy_of_vaporization_vjp: null required pointer"); e != GO_ON)
        return e;
    if (((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(g_params)) & 15) != 0)
        return fail_msg("pcs_pure_enthalpy_of_vaporization_vjp: params and g_params must be 16-byte aligned");
    const unsigned grid = grid_for(n, BLOCK);
    hipLaunchKernelGGL(k_pure_enthalpy_vjp, dim3(grid), dim3(BLOCK), 0, as_stream(stream), params, temp, rho_vl, n, g_dh, g_params,
                       g_temp);
    return launched("k_pure_enthalpy_vjp launch");
}

}  // extern "C"
