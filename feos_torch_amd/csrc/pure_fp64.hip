// The pure-component kernels built WITHOUT re-association (feos_torch_amd/build.py: RELAXED, no REASSOC): the all-fp64 VLE
// kernel and the liquid-density kernel, which -fassociative-math -freciprocal-math makes SLOWER (x0.96; 0.895 -> 1.19 ms: the
// re-associated expressions cost k_pure_liquid_density its register budget), behind two launch functions that
// pure_kernels.hip calls.  Measured in one process with scripts/dev/ab_bench.py / ab_k2.py / ab_purejac.py (round 3).
#include "abi_common.hpp"
#include "pure_vle_rows.hpp"

using namespace pcs_abi;

namespace {

// ------------------------------------------------------------------------------------------
// K2: liquid density at (T, p)
// ------------------------------------------------------------------------------------------
// liquid-density kernel: 204 VGPRs fit two waves per SIMD; held to 168 (52 spill instructions) three: 1.02 -> 0.89 ms per 1e7
// rows (four, 128 VGPRs: 1.02 ms)
constexpr int K2_WAVES = 3;
__global__ __launch_bounds__(STAGE_BLOCK, K2_WAVES) void k_pure_liquid_density(const double* __restrict__ params,
                                                               const double* __restrict__ temp,
                                                               const double* __restrict__ pressure, int64_t n,
                                                               double* __restrict__ rho_out,
                                                               double* __restrict__ rho_root,
                                                               uint8_t* __restrict__ status) {
    __shared__ double lds[STAGE_BLOCK * STAGE_ROW_PAD];
    const int64_t row0 = (int64_t)blockIdx.x * STAGE_BLOCK;
    // rows of the workgroup bucketed by class as in k_pure_vle (LDS counting sort): a wave mostly runs one set of
    // branches of the Helmholtz energy
    __shared__ int perm[STAGE_BLOCK];
    __shared__ int bins[K1_BINS];
    const int t = threadIdx.x;
    block_order_reset<K1_BINS>(bins);
    stage_rows(params, n, row0, lds);
    block_order_sort<K1_BINS>(bins, perm, [=] { return k1_bucket(&lds[t * STAGE_ROW_PAD]); });
    const int src = perm[t];
    double par[8];
#pragma unroll
    for (int q = 0; q < 8; q++) par[q] = lds[src * STAGE_ROW_PAD + q];
    const int64_t i = row0 + src;
    const bool live = i < n;
    const int64_t ii = live ? i : n - 1;
    const double T = temp[ii];
    const double p_red = pressure[ii] / (T * P_UNIT);  // pcsaft_pure.py:196

    PureCoef<double> c;
    pure_coef<double>(c, par, T, false);
    double rho;
    Eval last;
    int st = liquid_density_solve(c, p_red, TOL_STEP, rho, last);
    if (!live) return;
    // `rho` already carries the final Newton update rho - (p - p_spec)/dp (pcsaft_pure.py:198) taken
    // at a point whose relative step was <= TOL_STEP, i.e. it is converged to ~1e-11; it is both
    // the returned property and the density reported as the root.
    bool ok = (st == ST_OK);
    if (rho_out) rho_out[i] = ok ? rho * (1.0 / RHO_UNIT) : 0.0;
    if (rho_root) rho_root[i] = ok ? rho : 0.0;
    status[i] = ok ? 0 : 1;
}

}  // namespace

namespace pcs_abi {
int launch_pure_vle_full(const double* params, const double* temp, int64_t n, double* p_sat, double* rho_eq, double* rho_vl,
                         uint8_t* status, int32_t* iters, int32_t* retry, hipStream_t s) {
    hipLaunchKernelGGL(k_pure_vle<false>, dim3(grid_for(n, STAGE_BLOCK)), dim3(STAGE_BLOCK), 0, s, params, temp, n, p_sat, rho_eq, rho_vl, status,
                       iters, retry);
    return launched("k_pure_vle launch");
}
int launch_pure_liquid_density(const double* params, const double* temp, const double* pressure, int64_t n, double* rho_out,
                               double* rho_root, uint8_t* status, hipStream_t s) {
    hipLaunchKernelGGL(k_pure_liquid_density, dim3(grid_for(n, STAGE_BLOCK)), dim3(STAGE_BLOCK), 0, s, params, temp, pressure, n, rho_out, rho_root, status);
    return launched("k_pure_liquid_density launch");
}
}  // namespace pcs_abi
