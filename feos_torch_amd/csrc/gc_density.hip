// Liquid / vapour densities of gc-PC-SAFT rows at given (T, p, x) (see include/pcsaft_hip.h: pcs_gc_density; the per-lane
// routine is density_root of mix_density.hpp, instantiated here for GcModelT<double>).  Own translation unit, compiled like
// gc_kernels.hip with the guarded short logarithm and reciprocal (feos_torch_amd/build.py, GUARDED_SOURCES): the evaluation
// then has the arithmetic of pcs_gc_derivatives, and NaN / infinity semantics stay IEEE, which the bracketing and the
// failure detection rely on.  The backward pass is pcs_gc_derivatives_vjp at the root with a per-row weight on g_p
// (feos_torch_amd/gc_pcsaft.py, _GcDensity).
//
// Launch shape, that of k_gc_temperature: one row per lane, 128-thread workgroups, the table, the lanes' row bytes and bond
// diameters in LDS, rows in the caller's class order or bucketed by class inside the workgroup.  The row pick is the last
// place where a lane waits for another: behind it every lane runs its own root (at most DENS_MAX_EVALS evaluations), and a
// wave pays its slowest row.  A pure component (x = 0 or x = 1) is an ordinary row: gc_a is finite and regular at an exactly
// zero partial density, so the per-lane path has no special case for it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pcsaft_hip.h"
#include "abi_common.hpp"
#include "block_order.hpp"
#include "gc_model.hpp"
#include "gc_kernel_common.hpp"
#include "mix_density.hpp"

using namespace pcs;
using namespace pcs_abi;

namespace {

constexpr int GDBLOCK = 128;

__global__ __launch_bounds__(GDBLOCK) void k_gc_density(int phase, const double* __restrict__ table, int S,
                                                        const unsigned char* __restrict__ rows, const double* __restrict__ phi,
                                                        const double* __restrict__ temp, const double* __restrict__ pressure,
                                                        const double* __restrict__ x, int64_t n, double* __restrict__ rho_out,
                                                        double* __restrict__ dpdrho, uint8_t* __restrict__ status,
                                                        int32_t* __restrict__ iters, const int32_t* __restrict__ order) {
    extern __shared__ double lds[];
    GcTable tb = stage_table(table, S, lds);
    double* bonds = lds + gc_table_doubles(S);          // [2*MAXE][GDBLOCK]: the bond diameters d_ab
    double* row_area = bonds + 2 * GC_MAXE * GDBLOCK;   // the lanes' row bytes (stage_row)
    const int t = threadIdx.x;
    const int64_t i = gc_pick_row<GDBLOCK>(rows, tb, n, order);
    if (i >= n) return;  // (behind every barrier of the kernel)
    const double T = temp[i], p = pressure[i], x0 = x[i];
    const double ph0 = phi[2 * i], ph1 = phi[2 * i + 1];
    DensityResult r;
    r.rho = 0.0; r.dpdrho = 0.0; r.evals = 0;
    bool ok = is_finite_bits(T) && T > 0.0 && is_finite_bits(p) && p > 0.0 && is_finite_bits(x0) && x0 >= 0.0 && x0 <= 1.0 &&
              is_finite_bits(ph0) && is_finite_bits(ph1);
    if (ok) {  // lane-private from here on: an invalid row takes no part in any solve and no lane waits for it
        const unsigned char* row = stage_row(rows + (size_t)i * GC_ROW_BYTES, row_area);
        GcModelT<double> m;
        m.c.bond_dab = bonds + t;
        m.c.stride = GDBLOCK;
        gc_coef<double>(m.c, row, tb, ph0, ph1, T);
        ok = density_root(m, phase, x0, p / (T * P_UNIT), r) == 0 && is_finite_bits(r.rho) && is_finite_bits(r.dpdrho) && r.rho > 0.0;
    }
    if (rho_out) rho_out[i] = ok ? r.rho : 0.0;
    if (dpdrho) dpdrho[i] = ok ? r.dpdrho : 0.0;
    if (iters) iters[i] = ok ? r.evals : -1;
    status[i] = ok ? 0 : 1;
}

}  // namespace

extern "C" {

int pcs_gc_density(int phase, const double* table, int S, const uint8_t* rows, const double* phi, const double* temp,
                   const double* pressure, const double* x, int64_t n, double* rho, double* dpdrho, uint8_t* status,
                   int32_t* iters, const int32_t* order, void* stream) {
    if (int e = gc_enter(S, n, table && rows && phi && temp && pressure && x && status, "pcs_gc_density: null required pointer");
        e != GO_ON)
        return e;
    if (phase != DENS_LIQUID && phase != DENS_VAPOUR) return fail_msg("pcs_gc_density", "phase must be 0 (liquid) or 1 (vapour)");
    if (int e = aligned16("pcs_gc_density", "rows", rows)) return e;
    const size_t lds = gc_lds_bytes(S, GDBLOCK, 2 * GC_MAXE + GC_ROW_LDS_DOUBLES);
    hipLaunchKernelGGL(k_gc_density, dim3(grid_for(n, GDBLOCK)), dim3(GDBLOCK), lds, as_stream(stream), phase, table, S, rows, phi,
                       temp, pressure, x, n, rho, dpdrho, status, iters, order);
    return launched("k_gc_density launch");
}

}  // extern "C"
