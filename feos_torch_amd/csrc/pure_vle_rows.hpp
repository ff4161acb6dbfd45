// Stage 1 of the pure-component VLE as both pure units build it: the row body pure_vle_rows and the k_pure_vle kernel template.
// pure_kernels.hip (re-associated) instantiates the pressure-only forms, pure_fp64.hip (not re-associated) the all-fp64 one.
//
// Launch shape: one state point per lane, 256-thread workgroups (4 waves), grid = ceil(n/256)
// (>> 256 workgroups at the benchmark sizes, so all 8 XCDs fill; rows are independent, so the
// round-robin workgroup->XCD placement needs no remapping — there is no shared tile to keep
// in one L2).  HBM traffic is 81 B per state point against ~1e4 fp64 operations: the kernels
// are fp64-VALU bound; memory handling only has to be coalesced, which it is:
//   * the [n,8] AoS parameter rows of a workgroup (16 KB contiguous) are fetched with 16-byte
//     per-lane loads and staged through LDS (72-byte padded rows, conflict-free ds_read_b64);
//   * T, p and all outputs are SoA and accessed lane-contiguously.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_order.hpp"
#include "pure_solver.hpp"
#include "pure_stage.hpp"

namespace {

using namespace pcs;

// ------------------------------------------------------------------------------------------
// K1: pure VLE, fast path.  Rows that need the robust initialisation are appended to
// retry[1..]; retry[0] is the running count.
// ------------------------------------------------------------------------------------------
// waves per SIMD asked of the compiler for the all-fp64 instantiation (p_sat + densities): 210 VGPRs fit two; held to 128
// (152 spill instructions) four are resident and the kernel is 1.20 -> 0.96 ms per 1e7 rows (three: 1.00 ms)
constexpr int K1_WAVES = 4;
constexpr int K1_WAVES_LITE = 4;  // pressure-only instantiation: 122 VGPR, 4 waves per SIMD (without -fno-slp-vectorize: 168 VGPR, 3 waves)
constexpr int K1_BINS = 4;
// (Round 2 measured a block-level straggler exchange of the fp32 coupled iteration -- lanes not converged after two iterations
// parked in LDS and finished together by the first wave: 0.815 ms against 0.797 ms without it at 256 threads per workgroup,
// 0.834 ms at 512, 1.014 ms at 1024; the two barriers and the serial straggler wave cost more than the 1.4 iterations per
// wave they save.  Removed.)

// Staging of k_pure_vle_ordered: position pos of the batch holds row order[pos] (a tile-local permutation as
// pcs_pure_row_order writes it; a scheduling hint, every row's bits are the same wherever it is solved).  Lane t solves the
// row at position row0 + t.  Every entry is bounded by n before it is an index (a foreign or stale array must not fault; an
// entry out of range stands for its own position); positions past n clamp to position n - 1 and store nothing.  The
// workgroups of a tile share an XCD (bijective swizzle: hardware workgroup b runs on XCD b % 8 and takes the b / 8-th of
// that XCD's contiguous share of the grid), so that a tile's lines are fetched into one L2, its scattered stores merge
// there, and every XCD sees every class -- with the plain mapping workgroup k of every 8-workgroup stretch of a
// class-ordered tile lands on the same XCD and the XCDs that only ever get polar + associating rows set the launch's time
// (measured on host-permuted input: 0.92 of the unsorted batch without the grouping, 1.07-1.18 with it).
// Workgroup-uniform values (the swizzle, row0, the tile's share of order[]) come from blockIdx / gridDim alone and live in
// scalar registers; per-lane indices are 32 bits wide (the host's enter() returns for n == 0 and refuses n >= 2^31 before
// any launch, so n - 1 below is a valid row).  Each lane reads and bounds ONE entry of order[], that of its own position,
// fetches its own 64-byte row with four 16-byte loads off one address and stages it, with T, for itself: no exchange of
// indices between lanes and no workgroup barrier (the loads of a wave touch 64 lines instead of 16, which this kernel,
// bound by VALU issue, does not notice on the bench batch: profiles/ordered_stage.md).  The row and T still go through LDS:
// the solve re-reads the row there instead of holding it in registers, and T arrives as the LDS load it is in k_pure_vle.
// The wave-level fence keeps the compiler from forwarding the stores to the loads.  Both are load-bearing for the
// bit-for-bit pins (tests/test_pure_row_order_gpu.py, test_pure_ordered_stage_gpu.py, test_model_shell_gpu.py): this unit
// is built with -fassociative-math, and with T handed over in a register (a global load) the compiler orders the products
// T enters differently -- measured: p_sat moves in the last bit on 2.3 % of the rows; without the fence the row never
// reaches LDS and it is 3.9 %.  Do not remove the fence or the pad-slot T without re-running those tests.
// -> the row of lane t, -1 for a lane past n; its parameters and T are staged at lds[t * STAGE_ROW_PAD].
__device__ __forceinline__ int ordered_stage(const double* __restrict__ params, const double* __restrict__ temp, int64_t n,
                                             const int32_t* __restrict__ order, double* lds) {
    const unsigned t = threadIdx.x;
    const unsigned b = blockIdx.x, nwg = gridDim.x, xcd = b % 8u, q = nwg / 8u, rem = nwg % 8u;
    const unsigned wg = (xcd < rem ? xcd * (q + 1u) : rem * (q + 1u) + (xcd - rem) * q) + b / 8u;
    const unsigned rows = (unsigned)n, row0 = min(wg * (unsigned)STAGE_BLOCK, rows - 1u);
    const unsigned last = rows - 1u - row0;  // row n - 1 as a position of this tile
    const unsigned pos = min(t, last);
    const unsigned entry = (unsigned)(order + row0)[pos];
    const unsigned i = entry < rows ? entry : row0 + pos;  // one unsigned test bounds both sides
    const double2* src = reinterpret_cast<const double2*>(params) + (uint64_t)i * 4u;
    double* mine = lds + t * STAGE_ROW_PAD;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double2 v = src[k];
        mine[2 * k] = v.x;
        mine[2 * k + 1] = v.y;
    }
    mine[8] = temp[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    return t <= last ? (int)i : -1;
}

// Bucket key of a staged row: model class (which branches of the Helmholtz energy the row needs) in
// Gray order none, polar, polar+assoc, assoc -- neighbouring buckets share a branch.  Lanes of one
// wave then mostly run the same branches.  (A second key, a coarse reduced temperature as predictor of
// the iteration count, measured 0.5-1.5 % slower on a 256-row domain: not used.)
__device__ __forceinline__ int k1_bucket(const double* row) {
    const bool polar = row[3] != 0.0;
    const bool assoc = (row[4] != 0.0) && (row[6] != 0.0 || row[7] != 0.0);
    return polar ? (assoc ? 2 : 1) : (assoc ? 3 : 0);
}

// The 256 staged rows of the workgroup are bucketed (LDS counting sort; the order inside a bucket is
// irrelevant) and lane t solves the row at sorted position t.  A larger bucketing domain (4 tiles per
// workgroup) measured only 2-3 % faster and costs either LDS occupancy or a non-inlined call per
// tile whose callee-saved registers go through scratch (3.8 GB of HBM writes per 1e7 rows): not used.
// LITE (pressure-only output, fp32 pre-solve available): vle_fast_lite; rows without a usable fp32 result are
// appended with bit 31 set (k_pure_vle_fallback takes them), rows for the robust pass without.
// POLISH (with LITE): the densities are handed out (rho_eq / rho_vl) and take the exact Newton update of vle_lite_finish<true>
// RHO (with LITE, without POLISH; k_pure_vle_rho): rho_vl is handed out next to an unchanged p_sat (vle_polish_densities)
// ORDERED (with LITE, without POLISH and RHO; k_pure_vle_ordered): the rows come in the caller's tile-local order
// (pcs_pure_row_order), lane t solves the row at position t of it and nothing is sorted here: see ordered_stage.
template <bool LITE, bool POLISH, bool RHO, bool ORDERED = false>
__device__ __forceinline__ void pure_vle_rows(const double* __restrict__ params,
                                                    const double* __restrict__ temp, int64_t n,
                                                    double* __restrict__ p_sat, double* __restrict__ rho_eq,
                                                    double* __restrict__ rho_vl, uint8_t* __restrict__ status,
                                                    int32_t* __restrict__ iters, int32_t* __restrict__ retry,
                                                    const int32_t* __restrict__ order = nullptr) {
    __shared__ double lds[STAGE_BLOCK * STAGE_ROW_PAD];  // 8 parameters + T per row
    __shared__ int perm[STAGE_BLOCK];
    __shared__ int bins[K1_BINS];
    const int t = threadIdx.x;
    if constexpr (ORDERED) {
        const int row = ordered_stage(params, temp, n, order, lds);
        VleResult res;
        const double T = lds[t * STAGE_ROW_PAD + 8];
        const int st = vle_fast_lite<POLISH, RHO>(&lds[t * STAGE_ROW_PAD], T, res);
        if (row < 0) return;
        const unsigned i = (unsigned)row;
        if (st == ST_OK) {
            if (p_sat) p_sat[i] = res.p_star * T * P_UNIT;
            if (iters) iters[i] = res.iters;
            status[i] = 0;
        } else {
            status[i] = 1;  // provisional; a later pass overwrites it
            const int slot = atomicAdd(&retry[0], 1);
            if (slot >= 0 && slot < n) retry[1 + slot] = (int32_t)(i | (st == ST_FALLBACK ? 0x80000000u : 0u));
        }
        return;
    }
    const int64_t row0 = (int64_t)blockIdx.x * STAGE_BLOCK;
    // cooperative, coalesced staging as stage_rows (pure_stage.hpp), plus T (rows past n clamp to row n-1; never stored).  Written out,
    // like the result stores and list appends below (and in k_pure_vle_fallback): behind shared helpers, forced inline, the compiler
    // schedules all six VLE kernels differently (profiles/pure_split.md)
    {
        const double2* src = reinterpret_cast<const double2*>(params);
        const int64_t last2 = n * 4 - 1;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            int idx2 = t + k * STAGE_BLOCK;
            int64_t g = row0 * 4 + idx2;
            if (g > last2) g = last2 - 3 + (idx2 & 3);
            double2 v = src[g];
            int r = idx2 >> 2, c2 = idx2 & 3;
            lds[r * STAGE_ROW_PAD + 2 * c2] = v.x;
            lds[r * STAGE_ROW_PAD + 2 * c2 + 1] = v.y;
        }
        const int64_t g = row0 + t;
        lds[t * STAGE_ROW_PAD + 8] = temp[g < n ? g : n - 1];
        block_order_reset<K1_BINS>(bins);
    }
    __syncthreads();
    block_order_sort<K1_BINS>(bins, perm, [=] { return k1_bucket(&lds[t * STAGE_ROW_PAD]); });

    const int r = perm[t];
    const int64_t i = row0 + r;
    const bool live = i < n;
    double par[8];
#pragma unroll
    for (int q = 0; q < 8; q++) par[q] = lds[r * STAGE_ROW_PAD + q];
    const double T = lds[r * STAGE_ROW_PAD + 8];

    VleResult res;
    int st;  // every lane of the wave makes the call (its loops end on ballots over the lanes still working)
    const bool polish_rho = rho_vl != nullptr;  // densities as an output of a solve that stops at the pressure tolerances
    if (LITE) st = vle_fast_lite<POLISH, RHO>(&lds[r * STAGE_ROW_PAD], lds[r * STAGE_ROW_PAD + 8], res);  // the row is re-read from LDS for the fp64 coefficients
    else st = rho_eq ? vle_fast<true>(par, T, res, 1e-8, TOL_STEP) : vle_fast<true>(par, T, res, TOL_L_P, TOL_V_P, polish_rho);

    if (!live) return;
    if (st == ST_OK) {
        if (p_sat) p_sat[i] = res.p_star * T * P_UNIT;
        if (rho_eq) rho_eq[i] = res.rho_l * (1.0 / RHO_UNIT);
        if (rho_vl) {
            rho_vl[2 * i] = res.rho_v;
            rho_vl[2 * i + 1] = res.rho_l;
        }
        if (iters) iters[i] = res.iters;
        status[i] = 0;
    } else {
        status[i] = 1;  // provisional; a later pass overwrites it
        const int slot = atomicAdd(&retry[0], 1);
        // bounded append: a counter that was not reset (stale / foreign workspace) must not send the store out of the list
        if (slot >= 0 && slot < n) retry[1 + slot] = (int32_t)((uint32_t)i | (st == ST_FALLBACK ? 0x80000000u : 0u));  // n < 2^31 checked on the host
    }
}

template <bool LITE, bool POLISH = false>
__global__ __launch_bounds__(STAGE_BLOCK, LITE ? K1_WAVES_LITE : K1_WAVES) void k_pure_vle(const double* __restrict__ params,
                                                    const double* __restrict__ temp, int64_t n,
                                                    double* __restrict__ p_sat, double* __restrict__ rho_eq,
                                                    double* __restrict__ rho_vl, uint8_t* __restrict__ status,
                                                    int32_t* __restrict__ iters, int32_t* __restrict__ retry) {
    pure_vle_rows<LITE, POLISH, false>(params, temp, n, p_sat, rho_eq, rho_vl, status, iters, retry);
}

}  // namespace
