// Saturation pressure and saturated densities of ONE molecule of each gc-PC-SAFT row, taken as a pure fluid (see
// include/pcsaft_hip.h: pcs_gc_pure_vle; the per-lane routine is pure_line_vle of gc_saturation.hpp, instantiated here for
// GcModelT<double>).  Own translation unit, compiled like gc_density.hip with the guarded short logarithm and reciprocal
// (feos_torch_amd/build.py, GUARDED_SOURCES): the evaluation then has the arithmetic of pcs_gc_derivatives, and NaN / infinity
// semantics stay IEEE, which the failure detection relies on.  The backward pass needs no kernel of its own: two
// pcs_gc_derivatives_vjp calls, one per phase, with weights on a and p (feos_torch_amd/gc_pcsaft.py, _GcSaturation).
//
// Launch shape, that of k_gc_density: one row per lane, 128-thread workgroups, the table, the lanes' row bytes and bond
// diameters in LDS, rows in the caller's class order or bucketed by class inside the workgroup.  The row pick is the last
// place where a lane waits for another: behind it every lane runs its own solve, and a wave pays its slowest row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pcsaft_hip.h"
#include "abi_common.hpp"
#include "block_order.hpp"
#include "gc_model.hpp"
#include "gc_kernel_common.hpp"
#include "gc_saturation.hpp"

using namespace pcs;
using namespace pcs_abi;

namespace {

constexpr int GSBLOCK = 128;

__global__ __launch_bounds__(GSBLOCK) void k_gc_pure_vle(int component, const double* __restrict__ table, int S,
                                                         const unsigned char* __restrict__ rows, const double* __restrict__ phi,
                                                         const double* __restrict__ temp, int64_t n, double* __restrict__ p_sat,
                                                         double* __restrict__ rho_vl, double* __restrict__ dpdrho_vl,
                                                         uint8_t* __restrict__ status, int32_t* __restrict__ iters,
                                                         const int32_t* __restrict__ order) {
    extern __shared__ double lds[];
    GcTable tb = stage_table(table, S, lds);
    double* bonds = lds + gc_table_doubles(S);          // [2*MAXE][GSBLOCK]: the bond diameters d_ab
    double* row_area = bonds + 2 * GC_MAXE * GSBLOCK;   // the lanes' row bytes (stage_row)
    const int t = threadIdx.x;
    const int64_t i = gc_pick_row<GSBLOCK>(rows, tb, n, order);
    if (i >= n) return;  // (behind every barrier of the kernel)
    const double T = temp[i];
    const double ph0 = phi[2 * i], ph1 = phi[2 * i + 1];
    SatResult r;
    r.p_star = r.rho_v = r.rho_l = r.dp_v = r.dp_l = 0.0;
    int evals = 0;
    bool ok = is_finite_bits(T) && T > 0.0 && is_finite_bits(ph0) && is_finite_bits(ph1);
    if (ok) {  // lane-private from here on: an invalid row takes no part in any solve and no lane waits for it
        const unsigned char* row = stage_row(rows + (size_t)i * GC_ROW_BYTES, row_area);
        GcModelT<double> m;
        m.c.bond_dab = bonds + t;
        m.c.stride = GSBLOCK;
        gc_coef<double>(m.c, row, tb, ph0, ph1, T);
        ok = pure_line_vle(m, component, r, evals) == 0;
        const double p = r.p_star * T * P_UNIT;
        ok = ok && is_finite_bits(p) && p > 0.0 && is_finite_bits(r.rho_v) && is_finite_bits(r.rho_l) && is_finite_bits(r.dp_v) &&
             is_finite_bits(r.dp_l);
        r.p_star = p;
    }
    if (p_sat) p_sat[i] = ok ? r.p_star : 0.0;
    if (rho_vl) {
        rho_vl[2 * i] = ok ? r.rho_v : 0.0;
        rho_vl[2 * i + 1] = ok ? r.rho_l : 0.0;
    }
    if (dpdrho_vl) {
        dpdrho_vl[2 * i] = ok ? r.dp_v : 0.0;
        dpdrho_vl[2 * i + 1] = ok ? r.dp_l : 0.0;
    }
    if (iters) iters[i] = ok ? evals : -1;
    status[i] = ok ? 0 : 1;
}

}  // namespace

extern "C" {

int pcs_gc_pure_vle(int component, const double* table, int S, const uint8_t* rows, const double* phi, const double* temp,
                    int64_t n, double* p_sat, double* rho_vl, double* dpdrho_vl, uint8_t* status, int32_t* iters,
                    const int32_t* order, void* stream) {
    if (int e = gc_enter(S, n, table && rows && phi && temp && status, "pcs_gc_pure_vle: null required pointer"); e != GO_ON)
        return e;
    if (component != 0 && component != 1) return fail_msg("pcs_gc_pure_vle", "component must be 0 or 1 (molecule index)");
    if (int e = aligned16("pcs_gc_pure_vle", "rows", rows)) return e;
    const size_t lds = gc_lds_bytes(S, GSBLOCK, 2 * GC_MAXE + GC_ROW_LDS_DOUBLES);
    hipLaunchKernelGGL(k_gc_pure_vle, dim3(grid_for(n, GSBLOCK)), dim3(GSBLOCK), lds, as_stream(stream), component, table, S, rows,
                       phi, temp, n, p_sat, rho_vl, dpdrho_vl, status, iters, order);
    return launched("k_gc_pure_vle launch");
}

}  // extern "C"
