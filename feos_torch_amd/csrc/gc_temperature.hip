// Bubble / dew temperatures of gc-PC-SAFT rows at given pressures (see include/pcsaft_hip.h:
// pcs_gc_bubble_dew_temperature; the per-lane routine is gc_temperature.hpp on the outer iteration of mix_temperature.hpp).
// Own translation unit, compiled like gc_kernels.hip with the guarded short logarithm and reciprocal (feos_torch_amd/build.py,
// GUARDED_SOURCES): the cold trial then has the arithmetic of pcs_gc_bubble_dew, so the pressure GcPcSaftMix.bubble_point
// returns at the solved temperature is the specified one to the rounding of the solver; NaN / infinity semantics stay IEEE,
// which the bracketing and the failure detection of the outer iteration rely on.  The backward pass is pcs_gc_jacobian and
// pcs_gc_segment_gradient at the solved state (feos_torch_amd/gc_pcsaft.py).
//
// Launch shape of k_gc_bubble_dew's single pass: one row per lane, 128-thread workgroups, the table, the lanes' row bytes
// and bond diameters in LDS, rows in the caller's class order or bucketed by class inside the workgroup.  No work queue: a
// wave pays its slowest row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pcsaft_hip.h"
#include "abi_common.hpp"
#include "block_order.hpp"
#include "gc_model.hpp"
#include "gc_kernel_common.hpp"
#include "gc_temperature.hpp"

using namespace pcs;
using namespace pcs_abi;

namespace {

constexpr int GTBLOCK = 128;

template <bool DEW>
__global__ __launch_bounds__(GTBLOCK) void k_gc_temperature(const double* __restrict__ table, int S,
                                                            const unsigned char* __restrict__ rows,
                                                            const double* __restrict__ phi, const double* __restrict__ p_spec,
                                                            const double* __restrict__ z, const double* __restrict__ t_init,
                                                            int64_t n, double* __restrict__ t_out, double* __restrict__ rho4,
                                                            uint8_t* __restrict__ status, int32_t* __restrict__ iters,
                                                            const int32_t* __restrict__ order) {
    extern __shared__ double lds[];
    GcTable tb = stage_table(table, S, lds);
    double* bonds = lds + gc_table_doubles(S);          // [2*MAXE][GTBLOCK]: the bond diameters d_ab
    double* row_area = bonds + 2 * GC_MAXE * GTBLOCK;   // the lanes' row bytes (stage_row)
    const int t = threadIdx.x;
    const int64_t i = gc_pick_row<GTBLOCK>(rows, tb, n, order);
    if (i >= n) return;  // (behind every barrier of the kernel)
    const unsigned char* row = stage_row(rows + (size_t)i * GC_ROW_BYTES, row_area);
    double ph0 = phi[2 * i], ph1 = phi[2 * i + 1], zz = z[i];
    const double ps = p_spec[i], t0 = t_init[i];
    const bool fail = !(is_finite_bits(ps) && ps > 0.0) || !(is_finite_bits(t0) && t0 > 0.0) ||
                      !(is_finite_bits(zz) && zz > 0.0 && zz < 1.0) || !is_finite_bits(ph0) || !is_finite_bits(ph1);
    if (fail) {
        // a harmless state for the wave-uniform code (the lane's own structure row; T = 300 K inside the outer iteration); the
        // lane takes no part in any solve
        ph0 = ph1 = 1.0;
        zz = 0.5;
    }
    GcModelT<double> m;
    m.c.bond_dab = bonds + t;
    m.c.stride = GTBLOCK;
    MixTempResult r;
    const bool ok = gc_temperature<DEW>(m, row, tb, ph0, ph1, zz, ps, t0, fail, r) == 0;
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

int pcs_gc_bubble_dew_temperature(int dew, const double* table, int S, const uint8_t* rows, const double* phi, const double* p_spec,
                                  const double* z, const double* t_init, int64_t n, double* t_out, double* rho4, uint8_t* status,
                                  int32_t* iters, const int32_t* order, void* stream) {
    if (int e = gc_enter(S, n, table && rows && phi && p_spec && z && t_init && status, "pcs_gc_bubble_dew_temperature: null required pointer");
        e != GO_ON)
        return e;
    if (int e = aligned16("pcs_gc_bubble_dew_temperature", "rows and rho4", rows, rho4)) return e;
    const size_t lds = gc_lds_bytes(S, GTBLOCK, 2 * GC_MAXE + GC_ROW_LDS_DOUBLES);
    const dim3 grid(grid_for(n, GTBLOCK)), block(GTBLOCK);
    hipStream_t s = as_stream(stream);
    if (dew) hipLaunchKernelGGL(k_gc_temperature<true>, grid, block, lds, s, table, S, rows, phi, p_spec, z, t_init, n, t_out, rho4, status, iters, order);
    else hipLaunchKernelGGL(k_gc_temperature<false>, grid, block, lds, s, table, S, rows, phi, p_spec, z, t_init, n, t_out, rho4, status, iters, order);
    return launched("k_gc_temperature launch");
}

}  // extern "C"
