// Staging of a workgroup's [n,8] parameter rows through LDS: the one definition of the pure-component kernels' workgroup
// size, padded row and cooperative load (pure_kernels.hip, pure_fp64.hip, pure_critical.hip, pure_boiling.hip, pure_enthalpy.hip).
// 256-thread workgroups, 16-byte loads, 72-byte padded rows.  The pure VLE kernels (pure_vle_rows.hpp) keep a
// written-out copy of the load for their schedule's sake.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pcs {

constexpr int STAGE_BLOCK = 256;
constexpr int STAGE_ROW_PAD = 9;  // doubles per staged row (8 + 1 pad): bank-conflict-free per-lane reads

// Cooperative, coalesced load of the workgroup's parameter rows into lds[STAGE_BLOCK * STAGE_ROW_PAD], then a barrier.
// Rows past n are clamped to row n-1 (their results are never stored).
__device__ __forceinline__ void stage_rows(const double* __restrict__ params, int64_t n, int64_t row0, double* lds) {
    const int t = threadIdx.x;
    const double2* src = reinterpret_cast<const double2*>(params);
    const int64_t last2 = n * 4 - 1;  // index of the last double2
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int idx2 = t + k * STAGE_BLOCK;  // double2 index inside the block tile: row = idx2/4, col2 = idx2%4
        int64_t g = row0 * 4 + idx2;
        if (g > last2) g = last2 - 3 + (idx2 & 3);  // clamp to the same columns of row n-1
        const double2 v = src[g];
        const int r = idx2 >> 2, c2 = idx2 & 3;
        lds[r * STAGE_ROW_PAD + 2 * c2] = v.x;
        lds[r * STAGE_ROW_PAD + 2 * c2 + 1] = v.y;
    }
    __syncthreads();
}
// the same, then lane t's own row out of LDS
__device__ __forceinline__ void stage_rows(const double* __restrict__ params, int64_t n, int64_t row0, double* lds, double par[8]) {
    stage_rows(params, n, row0, lds);
#pragma unroll
    for (int k = 0; k < 8; k++) par[k] = lds[threadIdx.x * STAGE_ROW_PAD + k];
}

// Prologue of the kernels in which lane t takes row t of its workgroup: the staged parameter row, the row's index i,
// whether it exists (live), and the index ii to read the other inputs with (idle lanes repeat row n-1; they take part in
// the wave-uniform solver calls and store nothing).
struct LaneRow {
    double par[8];
    int64_t i, ii;
    bool live;
};
__device__ __forceinline__ LaneRow stage_lane_row(const double* __restrict__ params, int64_t n) {
    __shared__ double lds[STAGE_BLOCK * STAGE_ROW_PAD];
    const int64_t row0 = (int64_t)blockIdx.x * STAGE_BLOCK;
    LaneRow r;
    r.i = row0 + threadIdx.x;
    r.live = r.i < n;
    stage_rows(params, n, row0, lds, r.par);
    r.ii = r.live ? r.i : n - 1;
    return r;
}

}  // namespace pcs
