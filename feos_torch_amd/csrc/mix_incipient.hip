// Gradients of the bubble / dew pressure AND of the incipient-phase mole fraction at a converged binary bubble / dew point
// (see include/pcsaft_hip.h: pcs_mix_point_jacobian; the per-lane routine is mix_incipient.hpp).  Own translation unit,
// compiled with the flags of mix_kernels.hip (feos_torch_amd/build.py, GUARDED_SOURCES), whose k_mix_jacobian it stands
// next to: the backward pass of PcSaftMix.bubble_point / dew_point / bubble_temperature / dew_temperature with
// incipient_molefracs=True.  k_mix_jacobian itself is untouched and stays the backward pass of the default calls.
//
// Launch shape of k_mix_jacobian: one row per lane, 128-thread workgroups, rows in batch-wide class order when the caller
// brings a workspace, else bucketed by class inside the workgroup; ONE lane-strided adjoint block in LDS (61 doubles per
// lane, 62 KB per workgroup), used once per requested gradient.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pcsaft_hip.h"
#include "abi_common.hpp"
#include "block_order.hpp"
#include "mix_kernel_common.hpp"
#include "mix_incipient.hpp"

using namespace pcs;
using namespace pcs_abi;

namespace {

constexpr int MBLOCK = 128;

__global__ __launch_bounds__(MBLOCK) void k_mix_point_jacobian(int dew, const double* __restrict__ params,
                                                               const double* __restrict__ kij,
                                                               const double* __restrict__ temp,
                                                               const double* __restrict__ rho4, int64_t n,
                                                               double* __restrict__ jac_p, double* __restrict__ jac_y,
                                                               const int32_t* __restrict__ order) {
    __shared__ int perm[MBLOCK];
    __shared__ int bins[MIX_BINS + 1];
    __shared__ double adj_lds[ADJ_SLOTS * MBLOCK];  // coefficient adjoints of this lane's row: adj_lds[k * MBLOCK + t]
    const int t = threadIdx.x;
    const int64_t i = mix_pick_row<MBLOCK>(params, n, order, bins, perm);
    if (i >= n) return;
    double par[16], k0, k1;
    load_mix_row(params, kij, i, par, k0, k1);
    const double4 r = reinterpret_cast<const double4*>(rho4)[i];  // (V0, V1, L0, L1)
    double* gp = jac_p ? jac_p + MIX_DIRS * i : nullptr;
    double* gy = jac_y ? jac_y + MIX_DIRS * i : nullptr;
    double* adj = adj_lds + t;
    if (dew) mix_point_jacobian(par, k0, k1, temp[i], r.x, r.y, r.z, r.w, true, gp, gy, adj, MBLOCK);
    else mix_point_jacobian(par, k0, k1, temp[i], r.z, r.w, r.x, r.y, false, gp, gy, adj, MBLOCK);
}

}  // namespace

extern "C" {

int pcs_mix_point_jacobian(int dew, const double* params, const double* kij, const double* temp, const double* rho4,
                           int64_t n, double* jac_p, double* jac_y, void* workspace, void* stream) {
    if (int e = enter(n, params && kij && temp && rho4, "pcs_mix_point_jacobian: null required pointer"); e != GO_ON) return e;
    if (!jac_p && !jac_y) return fail_msg("pcs_mix_point_jacobian", "jac_p and jac_y are both null (one output is required)");
    hipStream_t s = as_stream(stream);
    const int32_t* order;  // batch-wide class order (the permutation of the work-queue schedule)
    if (int e = mix_class_order(params, n, workspace, s, order)) return e;
    hipLaunchKernelGGL(k_mix_point_jacobian, dim3(grid_for(n, MBLOCK)), dim3(MBLOCK), 0, s, dew, params, kij, temp, rho4, n,
                       jac_p, jac_y, order);
    return launched("k_mix_point_jacobian launch");
}

}  // extern "C"
