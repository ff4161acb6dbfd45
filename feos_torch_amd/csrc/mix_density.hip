// Liquid / vapour densities of binary-mixture rows at given (T, p, x) (see include/pcsaft_hip.h: pcs_mix_density; the
// per-lane routine is mix_density.hpp).  Own translation unit, compiled like mix_kernels.hip with the guarded short logarithm
// and reciprocal (feos_torch_amd/build.py, GUARDED_SOURCES): the evaluation then has the arithmetic of pcs_mix_derivatives,
// and NaN / infinity semantics stay IEEE, which the bracketing and the failure detection rely on.  The backward pass is
// pcs_mix_derivatives_vjp at the root with a per-row weight on g_p (feos_torch_amd/pcsaft_mix.py, _MixDensity).
//
// Launch shape: one row per lane in the rows' own order, 64-thread workgroups (one wave: ~16k waves per 1e6 rows spread
// evenly over the CUs, and a wave that ends early frees its slot at once), no LDS, no work queue, no waiting across lanes:
// a wave pays its slowest row, at most DENS_MAX_EVALS evaluations.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pcsaft_hip.h"
#include "abi_common.hpp"
#include "mix_kernel_common.hpp"
#include "mix_density.hpp"

using namespace pcs;
using namespace pcs_abi;

namespace {

constexpr int DBLOCK = 64;

__global__ __launch_bounds__(DBLOCK) void k_mix_density(int phase, const double* __restrict__ params, const double* __restrict__ kij,
                                                        const double* __restrict__ temp, const double* __restrict__ pressure,
                                                        const double* __restrict__ x, int64_t n, double* __restrict__ rho_out,
                                                        double* __restrict__ dpdrho, uint8_t* __restrict__ status,
                                                        int32_t* __restrict__ iters) {
    const int64_t i = (int64_t)blockIdx.x * DBLOCK + threadIdx.x;
    if (i >= n) return;
    const double T = temp[i], p = pressure[i], x0 = x[i];
    DensityResult r;
    r.rho = 0.0; r.dpdrho = 0.0; r.evals = 0;
    bool ok = is_finite_bits(T) && T > 0.0 && is_finite_bits(p) && p > 0.0 && is_finite_bits(x0) && x0 >= 0.0 && x0 <= 1.0;
    if (ok) {
        double par[16], k0, k1;
        load_mix_row(params, kij, i, par, k0, k1);
        MixModel m;
        mix_coef<double>(m.c, par, k0, k1, T);
        ok = density_root(m, phase, x0, p / (T * P_UNIT), r) == 0 && is_finite_bits(r.rho) && is_finite_bits(r.dpdrho) && r.rho > 0.0;
    }
    if (rho_out) rho_out[i] = ok ? r.rho : 0.0;
    if (dpdrho) dpdrho[i] = ok ? r.dpdrho : 0.0;
    if (iters) iters[i] = ok ? r.evals : -1;
    status[i] = ok ? 0 : 1;
}

}  // namespace

extern "C" {

int pcs_mix_density(int phase, const double* params, const double* kij, const double* temp, const double* pressure,
                    const double* x, int64_t n, double* rho, double* dpdrho, uint8_t* status, int32_t* iters,
                    void* workspace, void* stream) {
    if (int e = enter(n, params && kij && temp && pressure && x && status, "pcs_mix_density: null required pointer"); e != GO_ON) return e;
    if (phase != DENS_LIQUID && phase != DENS_VAPOUR) return fail_msg("pcs_mix_density", "phase must be 0 (liquid) or 1 (vapour)");
    if (int e = aligned16("pcs_mix_density", "params and kij", params, kij)) return e;
    // the batch-wide class order is accepted and NOT used: whether class-uniform waves pay for this kernel has not been
    // measured, and the pointer is in the signature so that using it later changes no caller
    (void)workspace;
    hipLaunchKernelGGL(k_mix_density, dim3(grid_for(n, DBLOCK)), dim3(DBLOCK), 0, as_stream(stream), phase, params, kij, temp,
                       pressure, x, n, rho, dpdrho, status, iters);
    return launched("k_mix_density launch");
}

}  // extern "C"
