// gfx950 kernels + C ABI for the heterosegmented gc-PC-SAFT path (GcPcSaftMix bubble / dew
// points and derivatives).  One state point per lane.  The per-batch segment / pair tables are
// staged into LDS by every workgroup; each lane keeps its bond list (d_ab, count) in a
// lane-strided LDS scratch area (conflict-free) so the hard-chain loop needs no registers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pcsaft_hip.h"
#include "abi_common.hpp"
#include "block_order.hpp"
#include "gc_model.hpp"
#include "gc_kernel_common.hpp"
#include "mix_solver.hpp"
#include "mix_solver_sm.hpp"

using namespace pcs;
using namespace pcs_abi;

namespace {

constexpr int GBLOCK = 128;

// fast-pass caps (mix_solver.hpp).  A/B on the synthetic dew batch (scripts/dev/ab_gc.py): 12/12: 9.0 ms, 6/8: 7.9, 4/8: 8.4, 7/7: 8.6
constexpr int GC_FAST_SS = 6, GC_FAST_NEWTON = 8;
constexpr int GC_RETRY_BLOCKS = 1024;
// (GC_NO_PROGRESS_DEW, GC_BINS and gc_bucket: gc_kernel_common.hpp, shared with gc_temperature.hip)

// (A work-queue schedule as in mix_kernels.hip was measured here too: the gc rows need nearly the same number of
// evaluations each, so it only adds the refill overhead: bubble 4.1 -> 4.7 ms, dew 12.4 -> 15.3 ms per 1e6 rows.)
// K7.  RETRY = false: fast pass over all rows (small caps, cap hits appended to the retry list;
// retry == nullptr -> full caps, single pass).  RETRY = true: robust pass, grid-stride over the list.
template <bool DEW, bool RETRY>
__global__ __launch_bounds__(GBLOCK) void k_gc_bubble_dew(const double* __restrict__ table, int S,
                                                          const unsigned char* __restrict__ rows,
                                                          const double* __restrict__ phi,
                                                          const double* __restrict__ temp, const double* __restrict__ z,
                                                          const double* __restrict__ p_init, int64_t n,
                                                          double* __restrict__ p_out, double* __restrict__ rho4,
                                                          uint8_t* __restrict__ status, int32_t* __restrict__ iters,
                                                          int32_t* __restrict__ retry, const int32_t* __restrict__ order) {
    extern __shared__ double lds[];
    if (RETRY && (int64_t)blockIdx.x * GBLOCK >= (int64_t)retry[0]) return;  // whole workgroup idle: skip the staging
    GcTable tb = stage_table(table, S, lds);
    double* bonds = lds + gc_table_doubles(S);  // [2*MAXE][GBLOCK]: the bond diameters d_ab
    double* row_area = bonds + 2 * GC_MAXE * GBLOCK;  // the lanes' row bytes (stage_row)
    GcModelT<double> m;
    m.c.bond_dab = bonds + threadIdx.x;
    m.c.stride = GBLOCK;
    int64_t first = (int64_t)blockIdx.x * GBLOCK + threadIdx.x;
    if constexpr (!RETRY) first = gc_pick_row<GBLOCK>(rows, tb, n, order);  // class-uniform waves
    const int64_t total = RETRY ? min((int64_t)max(retry[0], 0), n) : n;  // count and entries bounded by n: a foreign list must not fault
    const int64_t stride = RETRY ? (int64_t)gridDim.x * GBLOCK : total;  // fast pass: one row per lane
    for (int64_t k = first; k < total; k += stride) {
        const int64_t i = RETRY ? (int64_t)retry[1 + k] : k;
        if (RETRY && (i < 0 || i >= n)) continue;
        const double T = temp[i];
        gc_coef<double>(m.c, stage_row(rows + (size_t)i * GC_ROW_BYTES, row_area), tb, phi[2 * i], phi[2 * i + 1], T);
        MixResult r;
        const double p_red = p_init[i] / (T * P_UNIT);
        const bool fast = !RETRY && retry;
        bool root_failed = false;
        // dew: the pure-liquid fugacities of Raoult's law on the one-variable evaluation (5 of a row's ~20 two-variable
        // evaluations otherwise; round 3: dew 4.25 -> 4.02 ms per 1e6 rows)
        double fug[2], rho_pure[2];
        if (DEW) pure_fugacities_on_the_line(m, fug, rho_pure);
        // (may_damp = false: no damped second run of a failed Newton here -- mix_solver_sm.hpp::newton_failed.  The second pass
        // ends with its slowest row, and on the synthetic batch the damped run recovers 1 row per 1e6 for +0.2 ms.)
        // A row that fails at a liquid root with the full caps gets the robust second attempt (bracketed liquid roots,
        // mix_solver_sm.hpp): in the second pass, or in place when there is no work list.
        int rc;
        if constexpr (DEW) {
            rc = bubble_dew_solve_sm<DEW>(m, z[i], p_red, r, fast ? GC_FAST_SS : SS_MAX_IT, fast ? GC_FAST_NEWTON : NEWTON_MAX_IT, false,
                                          &root_failed, fug, rho_pure, false, GC_NO_PROGRESS_DEW);
            if (!fast && rc != BD_OK && root_failed)
                rc = bubble_dew_solve_sm<DEW>(m, z[i], p_red, r, SS_MAX_IT, NEWTON_MAX_IT, true, nullptr, nullptr, nullptr, false, GC_NO_PROGRESS_DEW);
        } else {
            (void)root_failed;
            rc = bubble_dew_solve_sm_both<DEW>(m, z[i], p_red, r, fast ? GC_FAST_SS : SS_MAX_IT, fast ? GC_FAST_NEWTON : NEWTON_MAX_IT, !fast,
                                               nullptr, nullptr, false);
        }
        if (fast && rc != BD_OK) {  // cap hit or failed: the second pass decides
            status[i] = 1;  // provisional
            const int slot = atomicAdd(&retry[0], 1);
            if (slot >= 0 && slot < n) retry[1 + slot] = (int32_t)i;  // bounded append (see pure_kernels.hip)
        } else {
            store_bubble_dew<DEW>(i, rc, r, T, p_out, rho4, status, iters);
        }
        if (!RETRY) break;
    }
}

// GcPcSaftMix.derivatives (feos_torch/gc_pcsaft.py:443-468)
__global__ __launch_bounds__(GBLOCK) void k_gc_derivatives(const double* __restrict__ table, int S,
                                                           const unsigned char* __restrict__ rows,
                                                           const double* __restrict__ phi,
                                                           const double* __restrict__ temp,
                                                           const double* __restrict__ rho, int64_t n,
                                                           double* __restrict__ a, double* __restrict__ p,
                                                           double* __restrict__ mu, double* __restrict__ v) {
    extern __shared__ double lds[];
    GcTable tb = stage_table(table, S, lds);
    double* bonds = lds + gc_table_doubles(S);
    const int64_t i = (int64_t)blockIdx.x * GBLOCK + threadIdx.x;
    if (i >= n) return;
    GcModelT<double> m;
    m.c.bond_dab = bonds + threadIdx.x;
    m.c.stride = GBLOCK;
    gc_coef<double>(m.c, stage_row(rows + (size_t)i * GC_ROW_BYTES, bonds + 2 * GC_MAXE * GBLOCK), tb, phi[2 * i], phi[2 * i + 1], temp[i]);
    PhaseEval e = phase_eval(m, rho[2 * i], rho[2 * i + 1]);
    if (a) a[i] = e.a;
    if (p) p[i] = e.p();
    if (mu) { mu[2 * i] = e.g0; mu[2 * i + 1] = e.g1; }
    if (v) {
        double d0 = e.dp0(), d1 = e.dp1();
        double den = 1.0 / (e.r0 * d0 + e.r1 * d1);
        v[2 * i] = d0 * den;
        v[2 * i + 1] = d1 * den;
    }
}

// fast pass over all rows and, with a work list, the robust pass over the rows it gave up on
template <bool DEW>
void launch_gc_bubble_dew(unsigned grid, size_t lds, hipStream_t s, const double* table, int S, const uint8_t* rows, const double* phi,
                          const double* temp, const double* z, const double* p_init, int64_t n, double* p_out, double* rho4,
                          uint8_t* status, int32_t* iters, int32_t* retry, const int32_t* order) {
    hipLaunchKernelGGL((k_gc_bubble_dew<DEW, false>), dim3(grid), dim3(GBLOCK), lds, s, table, S, rows, phi, temp, z, p_init, n, p_out,
                       rho4, status, iters, retry, order);
    if (retry)
        hipLaunchKernelGGL((k_gc_bubble_dew<DEW, true>), dim3(GC_RETRY_BLOCKS), dim3(GBLOCK), lds, s, table, S, rows, phi, temp, z,
                           p_init, n, p_out, rho4, status, iters, retry, order);
}

}  // namespace

extern "C" {

int64_t pcs_gc_table_doubles(int S) { return (int64_t)S * 8 + 3 * (int64_t)S * S; }

int pcs_gc_bubble_dew(int dew, const double* table, int S, const uint8_t* rows, const double* phi, const double* temp,
                      const double* z, const double* p_init, int64_t n, double* p_out, double* rho4, uint8_t* status,
                      int32_t* iters, const int32_t* order, void* workspace, void* stream) {
    if (int e = gc_enter(S, n, table && rows && phi && temp && z && p_init && status, "pcs_gc_bubble_dew: null required pointer"); e != GO_ON)
        return e;
    if (int e = aligned16("pcs_gc_bubble_dew", "rows", rows)) return e;
    const unsigned grid = grid_for(n, GBLOCK);
    const size_t lds = gc_lds_bytes(S, GBLOCK, 2 * GC_MAXE + GC_ROW_LDS_DOUBLES);
    hipStream_t s = as_stream(stream);
    int32_t* retry = static_cast<int32_t*>(workspace);
    if (retry) {
        if (int e = zero_ints(retry, 1, s)) return e;
    }
    (dew ? launch_gc_bubble_dew<true> : launch_gc_bubble_dew<false>)(grid, lds, s, table, S, rows, phi, temp, z, p_init, n, p_out, rho4, status,
                                                                     iters, retry, order);
    return launched("k_gc_bubble_dew launch");
}

int pcs_gc_derivatives(const double* table, int S, const uint8_t* rows, const double* phi, const double* temp,
                       const double* rho, int64_t n, double* a, double* p, double* mu, double* v, void* stream) {
    if (int e = gc_enter(S, n, table && rows && phi && temp && rho, "pcs_gc_derivatives: null required pointer"); e != GO_ON) return e;
    if (int e = aligned16("pcs_gc_derivatives", "rows", rows)) return e;
    const unsigned grid = grid_for(n, GBLOCK);
    hipLaunchKernelGGL(k_gc_derivatives, dim3(grid), dim3(GBLOCK), gc_lds_bytes(S, GBLOCK, 2 * GC_MAXE + GC_ROW_LDS_DOUBLES), as_stream(stream),
                       table, S, rows, phi, temp, rho, n, a, p, mu, v);
    return launched("k_gc_derivatives launch");
}

}  // extern "C"
