// Bubble / dew temperatures of binary-mixture rows at given pressures (see include/pcsaft_hip.h:
// pcs_mix_bubble_dew_temperature; the per-lane routine is mix_temperature.hpp).  Own translation unit, compiled like
// mix_kernels.hip with the guarded short logarithm and reciprocal (feos_torch_amd/build.py, GUARDED_SOURCES): the inner
// solve then has the arithmetic of pcs_mix_bubble_dew, so the pressure PcSaftMix.bubble_point returns at the solved
// temperature is the specified one to the rounding of the solver; NaN / infinity semantics stay IEEE, which the bracketing
// and the failure detection of the outer iteration rely on.  The backward pass is pcs_mix_jacobian at the solved state.
//
// Launch shape of k_mix_bubble_dew: one row per lane, 128-thread workgroups, rows bucketed by class inside the workgroup,
// or taken in batch-wide class order when the caller brings a workspace.  No work queue: a wave pays its slowest row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pcsaft_hip.h"
#include "abi_common.hpp"
#include "block_order.hpp"
#include "mix_kernel_common.hpp"
#include "mix_temperature.hpp"

using namespace pcs;
using namespace pcs_abi;

namespace {

constexpr int MBLOCK = 128;

template <bool DEW>
__global__ __launch_bounds__(MBLOCK, 1) void k_mix_temperature(const double* __restrict__ params, const double* __restrict__ kij,
                                                            const double* __restrict__ p_spec, const double* __restrict__ z,
                                                            const double* __restrict__ t_init, int64_t n,
                                                            double* __restrict__ t_out, double* __restrict__ rho4,
                                                            uint8_t* __restrict__ status, int32_t* __restrict__ iters,
                                                            const int32_t* __restrict__ order) {
    __shared__ int perm[MBLOCK];
    __shared__ int bins[MIX_BINS + 1];
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * MBLOCK;
    int64_t i;
    if (order) {
        if (row0 + t >= n) return;
        i = order[row0 + t];
        if (i < 0 || i >= n) return;
    } else {
        // rows past n sort last, in a bucket of their own
        block_order<MIX_BINS + 1>(bins, perm, [=] { return row0 + t < n ? mix_bucket(params + 16 * (row0 + t)) : MIX_BINS; });
        i = row0 + perm[t];
        if (i >= n) return;
    }
    double par[16], k0, k1;
    load_mix_row(params, kij, i, par, k0, k1);
    double zz = z[i];
    const double ps = p_spec[i], t0 = t_init[i];
    bool fail = !(is_finite_bits(ps) && ps > 0.0) || !(is_finite_bits(t0) && t0 > 0.0) || !(is_finite_bits(zz) && zz > 0.0 && zz < 1.0);
#pragma unroll
    for (int k = 0; k < 16; k++) fail = fail || !is_finite_bits(par[k]);
    fail = fail || !is_finite_bits(k0) || !is_finite_bits(k1);
    if (fail) {
        // a harmless row for the wave-uniform code (the row_or_idle of the pure units); the lane takes no part in any solve
#pragma unroll
        for (int k = 0; k < 16; k++) par[k] = 0.0;
        par[0] = par[8] = 1.5;
        par[1] = par[9] = 3.5;
        par[2] = par[10] = 250.0;
        k0 = k1 = 0.0;
        zz = 0.5;
    }
    MixModel m;
    MixTempResult r;
    const bool ok = mix_temperature<DEW>(m, par, k0, k1, zz, ps, t0, fail, r) == 0;
    if (t_out) t_out[i] = ok ? r.T : 0.0;
    if (rho4) {
        // reference layout: [rhoV_1, rhoV_2, rhoL_1, rhoL_2]
        const double v0 = DEW ? r.r.spec0 : r.r.inc0, v1 = DEW ? r.r.spec1 : r.r.inc1;
        const double l0 = DEW ? r.r.inc0 : r.r.spec0, l1 = DEW ? r.r.inc1 : r.r.spec1;
        double2* dst = reinterpret_cast<double2*>(rho4) + 2 * i;
        dst[0] = ok ? make_double2(v0, v1) : make_double2(0.0, 0.0);
        dst[1] = ok ? make_double2(l0, l1) : make_double2(0.0, 0.0);
    }
    if (iters) iters[i] = ok ? r.iters : -1;
    status[i] = ok ? 0 : 1;
}

}  // namespace

extern "C" {

int pcs_mix_bubble_dew_temperature(int dew, const double* params, const double* kij, const double* p_spec, const double* z,
                                   const double* t_init, int64_t n, double* t_out, double* rho4, uint8_t* status, int32_t* iters,
                                   void* workspace, void* stream) {
    if (int e = enter(n, params && kij && p_spec && z && t_init && status, "pcs_mix_bubble_dew_temperature: null required pointer"); e != GO_ON)
        return e;
    if (int e = aligned16("pcs_mix_bubble_dew_temperature", "params, kij and rho4", params, kij, rho4)) return e;
    hipStream_t s = as_stream(stream);
    const int32_t* order;  // batch-wide class order (the permutation of the work-queue schedule): class-uniform waves
    if (int e = mix_class_order(params, n, workspace, s, order)) return e;
    const dim3 grid(grid_for(n, MBLOCK)), block(MBLOCK);
    if (dew) hipLaunchKernelGGL(k_mix_temperature<true>, grid, block, 0, s, params, kij, p_spec, z, t_init, n, t_out, rho4, status, iters, order);
    else hipLaunchKernelGGL(k_mix_temperature<false>, grid, block, 0, s, params, kij, p_spec, z, t_init, n, t_out, rho4, status, iters, order);
    return launched("k_mix_temperature launch");
}

}  // extern "C"
