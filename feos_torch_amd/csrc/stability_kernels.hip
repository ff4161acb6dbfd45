// gfx950 kernels + C ABI of the tangent-plane stability analysis of binary feed states (stability.hpp): PcSaftMix and
// GcPcSaftMix rows, one row per lane.  Compiled with the guarded (IEEE NaN / infinity) flags of the solver units: the
// outcome of a row is decided by comparisons that must see NaN and infinity as such.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pcsaft_hip.h"
#include "abi_common.hpp"
#include "block_order.hpp"
#include "gc_kernel_common.hpp"
#include "mix_kernel_common.hpp"
#include "stability.hpp"

using namespace pcs;
using namespace pcs_abi;

namespace {

constexpr int SBLOCK = 128;

__device__ __forceinline__ void stab_store(int64_t i, const StabResult& r, double* __restrict__ tpd, double* __restrict__ rho_trial,
                                           uint8_t* __restrict__ status) {
    if (tpd) tpd[i] = r.tpd;
    if (rho_trial) reinterpret_cast<double2*>(rho_trial)[i] = make_double2(r.t0, r.t1);
    status[i] = (uint8_t)r.status;
}

__global__ __launch_bounds__(SBLOCK) void k_mix_stability(const double* __restrict__ params, const double* __restrict__ kij,
                                                          const double* __restrict__ temp, const double* __restrict__ rho,
                                                          int64_t n, double* __restrict__ tpd, double* __restrict__ rho_trial,
                                                          uint8_t* __restrict__ status) {
    // rows of the workgroup bucketed by class (LDS counting sort, as k_mix_bubble_dew): a wave mostly runs one set of
    // branches of the evaluation
    __shared__ int perm[SBLOCK];
    __shared__ int bins[MIX_BINS + 1];
    const int64_t i = mix_pick_row<SBLOCK>(params, n, nullptr, bins, perm);
    if (i >= n) return;
    double par[16], k0, k1;
    load_mix_row(params, kij, i, par, k0, k1);
    MixModel m;
    mix_coef<double>(m.c, par, k0, k1, temp[i]);
    const double2 r = reinterpret_cast<const double2*>(rho)[i];
    stab_store(i, stability_row(m, r.x, r.y), tpd, rho_trial, status);
}

__global__ __launch_bounds__(SBLOCK) void k_gc_stability(const double* __restrict__ table, int S, const unsigned char* __restrict__ rows,
                                                         const double* __restrict__ phi, const double* __restrict__ temp,
                                                         const double* __restrict__ rho, int64_t n, double* __restrict__ tpd,
                                                         double* __restrict__ rho_trial, uint8_t* __restrict__ status,
                                                         const int32_t* __restrict__ order) {
    extern __shared__ double lds[];
    GcTable tb = stage_table(table, S, lds);
    double* bonds = lds + gc_table_doubles(S);  // [2*MAXE][SBLOCK]: the bond diameters d_ab
    int64_t i = (int64_t)blockIdx.x * SBLOCK + threadIdx.x;
    if (i >= n) return;
    if (order) {  // class order of the rows (see pcs_gc_bubble_dew): only the schedule changes
        i = order[i];
        if (i < 0 || i >= n) return;
    }
    GcModelT<double> m;
    m.c.bond_dab = bonds + threadIdx.x;
    m.c.stride = SBLOCK;
    gc_coef<double>(m.c, stage_row(rows + (size_t)i * GC_ROW_BYTES, bonds + 2 * GC_MAXE * SBLOCK), tb, phi[2 * i], phi[2 * i + 1],
                    temp[i]);
    const double2 r = reinterpret_cast<const double2*>(rho)[i];
    stab_store(i, stability_row(m, r.x, r.y), tpd, rho_trial, status);
}

}  // namespace

extern "C" {

int pcs_mix_stability(const double* params, const double* kij, const double* temp, const double* rho, int64_t n, double* tpd,
                      double* rho_trial, uint8_t* status, void* stream) {
    if (int e = enter(n, params && kij && temp && rho && status, "pcs_mix_stability: null required pointer"); e != GO_ON) return e;
    const unsigned grid = grid_for(n, SBLOCK);
    hipLaunchKernelGGL(k_mix_stability, dim3(grid), dim3(SBLOCK), 0, as_stream(stream), params, kij, temp, rho, n, tpd, rho_trial,
                       status);
    return launched("k_mix_stability launch");
}

int pcs_gc_stability(const double* table, int S, const uint8_t* rows, const double* phi, const double* temp, const double* rho,
                     int64_t n, double* tpd, double* rho_trial, uint8_t* status, const int32_t* order, void* stream) {
    if (int e = gc_enter(S, n, table && rows && phi && temp && rho && status, "pcs_gc_stability: null required pointer"); e != GO_ON) return e;
    if (int e = aligned16("pcs_gc_stability", "rows", rows)) return e;
    const unsigned grid = grid_for(n, SBLOCK);
    hipLaunchKernelGGL(k_gc_stability, dim3(grid), dim3(SBLOCK), gc_lds_bytes(S, SBLOCK, 2 * GC_MAXE + GC_ROW_LDS_DOUBLES),
                       as_stream(stream), table, S, rows, phi, temp, rho, n, tpd, rho_trial, status, order);
    return launched("k_gc_stability launch");
}

}  // extern "C"
