// Boiling temperatures of pure-component parameter rows at given pressures (see include/pcsaft_hip.h:
// pcs_pure_boiling_temperature; solver in pure_boiling.hpp).  Own translation unit, compiled with strict IEEE semantics like
// pure_critical.hip and pure_robust.hip: the bracketing of the temperature and the failure detection rely on IEEE
// comparisons, and the unit has no fp32 pre-solve (feos_torch_amd/build.py).  The backward pass is the Jacobian kernel with
// selector 3 (pure_jacobian.hpp, pure_kernels.hip).
//
// Launch shape as the other pure kernels: one row per lane, 256-thread workgroups, the [n,8] parameter rows of a workgroup
// fetched with 16-byte loads and staged through LDS (pure_stage.hpp); pressure, T, status are SoA, the densities [n,2].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pcsaft_hip.h"
#include "abi_common.hpp"
#include "pure_boiling.hpp"
#include "pure_stage.hpp"

using namespace pcs;
using namespace pcs_abi;

namespace {

constexpr int BLOCK = STAGE_BLOCK;
constexpr int ROW_PAD = STAGE_ROW_PAD;

__global__ __launch_bounds__(BLOCK) void k_pure_boiling(const double* __restrict__ params, const double* __restrict__ pressure,
                                                        const double* __restrict__ t_init, int64_t n, double* __restrict__ temp,
                                                        double* __restrict__ rho_vl, uint8_t* __restrict__ status,
                                                        int32_t* __restrict__ iters) {
    __shared__ double lds[BLOCK * ROW_PAD];
    const int64_t row0 = (int64_t)blockIdx.x * BLOCK;
    const int64_t i = row0 + threadIdx.x;
    const bool live = i < n;
    stage_rows(params, n, row0, lds);
    double par[8];
#pragma unroll
    for (int k = 0; k < 8; k++) par[k] = lds[threadIdx.x * ROW_PAD + k];
    const int64_t ii = live ? i : n - 1;  // rows past n repeat row n-1 and are never stored
    BoilResult r;
    const int st = boiling_temperature(par, pressure[ii], t_init ? t_init[ii] : 0.0, t_init != nullptr, r);  // wave-uniform call
    if (!live) return;
    const bool ok = st == 0;
    if (temp) temp[i] = ok ? r.T : 0.0;
    if (rho_vl) {
        rho_vl[2 * i] = ok ? r.rho_v : 0.0;
        rho_vl[2 * i + 1] = ok ? r.rho_l : 0.0;
    }
    if (iters) iters[i] = ok ? r.iters : -1;
    status[i] = ok ? 0 : 1;
}

}  // namespace

extern "C" {

int pcs_pure_boiling_temperature(const double* params, const double* pressure, const double* t_init, int64_t n, double* temp,
                                 double* rho_vl, uint8_t* status, int32_t* iters, void* stream) {
    if (int e = enter(n, params && pressure && status, "pcs_pure_boiling_temperature: null required pointer"); e != GO_ON) return e;
    if ((reinterpret_cast<uintptr_t>(params) & 15) != 0) return fail_msg("pcs_pure_boiling_temperature: params must be 16-byte aligned");
    const unsigned grid = grid_for(n, BLOCK);
    hipLaunchKernelGGL(k_pure_boiling, dim3(grid), dim3(BLOCK), 0, as_stream(stream), params, pressure, t_init, n, temp, rho_vl,
                       status, iters);
    return launched("k_pure_boiling launch");
}

}  // extern "C"
