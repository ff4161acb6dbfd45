// Helpers shared by the binary-mixture translation units (mix_kernels.hip, mix_temperature.hip, mix_incipient.hip,
// stability_kernels.hip): the model struct the solvers are instantiated on, the row load, the class key of a parameter row,
// the row a lane works on (mix_pick_row) and the host side of the batch-wide class order (mix_class_order).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_order.hpp"
#include "mix_model.hpp"

namespace pcs_abi {
// batch-wide class order of the rows (mix_kernels.hip): perm[n] + control block in a workspace of pcs_workspace_bytes(n)
int launch_mix_class_order(const double* params, int64_t n, void* workspace, hipStream_t s);

// The `order` argument of the kernels that take their rows in class order when the caller brings a workspace: launches the
// class order into it (0, or the error of that launch sequence); order = null without a workspace.
inline int mix_class_order(const double* params, int64_t n, void* workspace, hipStream_t s, const int32_t*& order) {
    order = static_cast<const int32_t*>(workspace);
    return workspace ? launch_mix_class_order(params, n, workspace, s) : 0;
}
}  // namespace pcs_abi

namespace {

using namespace pcs;

struct MixModel {
    MixCoef<double> c;
    template <class R> PCS_DEV R a(const R& r0, const R& r1) const { return mix_a<double, R>(c, r0, r1); }
    template <class R, class Z> PCS_DEV R a_z(const R& r0, const R& r1, const Z& zeta3) const { return mix_a_z<double, R, Z>(c, r0, r1, zeta3); }
    PCS_DEV double packing(double x0, double x1) const { return x0 * c.zk[3][0] + x1 * c.zk[3][1]; }
};

__device__ __forceinline__ void load_mix_row(const double* __restrict__ params, const double* __restrict__ kij,
                                             int64_t i, double par[16], double& k0, double& k1) {
    const double2* src = reinterpret_cast<const double2*>(params + 16 * i);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        double2 v = src[k];
        par[2 * k] = v.x;
        par[2 * k + 1] = v.y;
    }
    double2 kk = reinterpret_cast<const double2*>(kij)[i];
    k0 = kk.x;
    k1 = kk.y;
}

constexpr int MIX_BINS = 8;
// association class (none, self, induced, cross: mix_model.hpp) x polarity of a parameter row [2][8]
__device__ __forceinline__ int mix_bucket(const double* __restrict__ row) {
    const double na0 = row[6], nb0 = row[7], na1 = row[14], nb1 = row[15];
    const int associating = (na0 + nb0 != 0.0) + (na1 + nb1 != 0.0);
    const int self_assoc = (na0 * nb0 != 0.0) + (na1 * nb1 != 0.0);
    int cls = 0;
    if (associating == 1 && self_assoc == 1) cls = 1;
    if (associating == 2 && self_assoc == 1) cls = 2;
    if (associating == 2 && self_assoc == 2) cls = 3;
    const int polar = (row[3] != 0.0) || (row[11] != 0.0);
    return 2 * cls + polar;
}

// The row this lane of a BLOCK-thread workgroup works on, or n for none.  With `order` (batch-wide class order of the
// caller's workspace, mix_class_order below) its entry, bounds-checked: a foreign order array must not fault.  Without:
// the rows of the workgroup bucketed by class (LDS counting sort in the kernel's bins[MIX_BINS + 1] / perm[BLOCK]) so that
// the lanes of a wave mostly run the same branches of the Helmholtz energy -- the cross-association site-fraction solve
// costs ~5x the rest of an evaluation and would otherwise be paid by every wave; rows past n sort last, in a bucket of
// their own.  `order` is the same for the whole grid, so either every lane of a workgroup reaches the barriers or none.
template <int BLOCK>
__device__ __forceinline__ int64_t mix_pick_row(const double* __restrict__ params, int64_t n, const int32_t* __restrict__ order,
                                                int* bins, int* perm) {
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * BLOCK;
    if (order) {
        if (row0 + t >= n) return n;
        const int64_t i = order[row0 + t];
        return (i < 0 || i >= n) ? n : i;
    }
    block_order<MIX_BINS + 1>(bins, perm, [=] { return row0 + t < n ? mix_bucket(params + 16 * (row0 + t)) : MIX_BINS; });
    const int64_t i = row0 + perm[t];
    return i >= n ? n : i;
}

}  // namespace
