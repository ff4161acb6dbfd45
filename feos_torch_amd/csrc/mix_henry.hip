// Henry's law constants of binary-mixture rows: the solute at infinite dilution in the pure, saturated solvent (see
// include/pcsaft_hip.h: pcs_mix_henry; the per-lane routine is mix_henry.hpp).  Own translation unit, compiled with strict
// IEEE semantics like pure_enthalpy.hip, whose saturated-state solve it shares: the failure detection relies on IEEE
// comparisons and there is no fp32 pre-solve (feos_torch_amd/build.py).  The backward pass needs no kernel of its own:
// pcs_mix_derivatives_vjp at (rho_L, 0) and pcs_pure_jacobian_vjp (selector 2) on the solvent row, weighted with this
// kernel's dlnh_drho (feos_torch_amd/pcsaft_mix.py, _MixHenry).
//
// Launch shape: one row per lane in the rows' own order, 64-thread workgroups (one wave, as k_mix_density), no LDS.  Lanes
// past n repeat row n-1 through the wave-uniform solver loops and store nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pcsaft_hip.h"
#include "abi_common.hpp"
#include "mix_kernel_common.hpp"
#include "mix_henry.hpp"

using namespace pcs;
using namespace pcs_abi;

namespace {

constexpr int HBLOCK = 64;

__global__ __launch_bounds__(HBLOCK) void k_mix_henry(int solute, const double* __restrict__ params, const double* __restrict__ kij,
                                                      const double* __restrict__ temp, int64_t n, double* __restrict__ h,
                                                      double* __restrict__ rho_vl, double* __restrict__ p_sat,
                                                      double* __restrict__ dlnh_drho, uint8_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * HBLOCK + threadIdx.x;
    const bool live = i < n;
    const int64_t ii = live ? i : n - 1;
    double par[16], k0, k1;
    load_mix_row(params, kij, ii, par, k0, k1);
    HenryResult r;
    const int st = henry_constant<MixModel>(par, k0, k1, temp[ii], solute, r);  // wave-uniform call
    if (!live) return;
    const bool ok = st == 0;
    h[i] = ok ? r.h : 0.0;
    if (rho_vl) {
        rho_vl[2 * i] = ok ? r.rho_v : 0.0;
        rho_vl[2 * i + 1] = ok ? r.rho_l : 0.0;
    }
    if (p_sat) p_sat[i] = ok ? r.p_sat : 0.0;
    if (dlnh_drho) dlnh_drho[i] = ok ? r.dlnh_drho : 0.0;
    status[i] = ok ? 0 : 1;
}

}  // namespace

extern "C" {

int pcs_mix_henry(int solute, const double* params, const double* kij, const double* temp, int64_t n, double* h, double* rho_vl,
                  double* p_sat, double* dlnh_drho, uint8_t* status, void* stream) {
    if (int e = enter(n, params && kij && temp && h && status, "pcs_mix_henry: null required pointer"); e != GO_ON) return e;
    if (solute != 0 && solute != 1) return fail_msg("pcs_mix_henry", "solute must be 0 or 1 (component index)");
    if (int e = aligned16("pcs_mix_henry", "params and kij", params, kij)) return e;
    hipLaunchKernelGGL(k_mix_henry, dim3(grid_for(n, HBLOCK)), dim3(HBLOCK), 0, as_stream(stream), solute, params, kij, temp, n, h,
                       rho_vl, p_sat, dlnh_drho, status);
    return launched("k_mix_henry launch");
}

}  // extern "C"
