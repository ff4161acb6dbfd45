// Boiling temperatures of pure-component parameter rows at given pressures (see include/pcsaft_hip.h:
// pcs_pure_boiling_temperature; solver in pure_boiling.hpp).  Own translation unit, compiled with strict IEEE semantics like
// pure_critical.hip and pure_robust.hip: the bracketing of the temperature and the failure detection rely on IEEE
// comparisons, and the unit has no fp32 pre-solve (feos_torch_amd/build.py).  The backward pass is the Jacobian kernel with
// selector 3 (pure_jacobian.hpp, pure_kernels.hip).
//
// Launch shape as the other pure kernels: one row per lane, 256-thread workgroups, the [n,8] parameter rows of a workgroup
// fetched with 16-byte loads and staged through LDS (stage_lane_row, pure_stage.hpp); pressure, T, status are SoA, the densities [n,2].
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

__global__ __launch_bounds__(BLOCK) void k_pure_boiling(const double* __restrict__ params, const double* __restrict__ pressure,
                                                        const double* __restrict__ t_init, int64_t n, double* __restrict__ temp,
                                                        double* __restrict__ rho_vl, uint8_t* __restrict__ status,
                                                        int32_t* __restrict__ iters) {
    const LaneRow row = stage_lane_row(params, n);  // pure_stage.hpp: rows past n repeat row n-1 and are never stored
    const int64_t i = row.i, ii = row.ii;
    BoilResult r;
    const int st = boiling_temperature(row.par, pressure[ii], t_init ? t_init[ii] : 0.0, t_init != nullptr, r);  // wave-uniform call
    if (!row.live) return;
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
    if (int e = aligned16("pcs_pure_boiling_temperature", "params", params)) return e;
    const unsigned grid = grid_for(n, BLOCK);
    hipLaunchKernelGGL(k_pure_boiling, dim3(grid), dim3(BLOCK), 0, as_stream(stream), params, pressure, t_init, n, temp, rho_vl,
                       status, iters);
    return launched("k_pure_boiling launch");
}

}  // extern "C"
