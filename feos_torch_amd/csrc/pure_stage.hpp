// Staging of a workgroup's [n,8] parameter rows through LDS, shared by the strict-IEEE pure-component units
// (pure_critical.hip, pure_boiling.hip): 256-thread workgroups, 16-byte loads, 72-byte padded rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pcs {

constexpr int STAGE_BLOCK = 256;
constexpr int STAGE_ROW_PAD = 9;  // doubles per staged row (8 + 1 pad): bank-conflict-free per-lane reads

// rows past n are clamped to row n-1 (their results are never stored)
__device__ __forceinline__ void stage_rows(const double* __restrict__ params, int64_t n, int64_t row0, double* lds) {
    const int t = threadIdx.x;
    const double2* src = reinterpret_cast<const double2*>(params);
    const int64_t last2 = n * 4 - 1;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int idx2 = t + k * STAGE_BLOCK;
        int64_t g = row0 * 4 + idx2;
        if (g > last2) g = last2 - 3 + (idx2 & 3);
        const double2 v = src[g];
        const int r = idx2 >> 2, c2 = idx2 & 3;
        lds[r * STAGE_ROW_PAD + 2 * c2] = v.x;
        lds[r * STAGE_ROW_PAD + 2 * c2 + 1] = v.y;
    }
    __syncthreads();
}

}  // namespace pcs
