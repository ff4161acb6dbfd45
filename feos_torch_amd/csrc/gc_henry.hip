// Henry's law constants of gc-PC-SAFT rows: one molecule of the row at infinite dilution in the other, pure and saturated (see
// include/pcsaft_hip.h: pcs_gc_henry; the two per-lane stages are gc_henry.hpp).  Own translation unit, compiled like
// gc_saturation.hip with the guarded short logarithm and reciprocal (feos_torch_amd/build.py, GUARDED_SOURCES): stage 1 then has
// the arithmetic of pcs_gc_pure_vle and stage 2 that of pcs_gc_derivatives, and NaN / infinity semantics stay IEEE, which the
// failure detection relies on.  The backward pass needs no kernel of its own: two pcs_gc_derivatives_vjp calls with weights on
// a, p and mu_s (feos_torch_amd/gc_pcsaft.py, _GcHenry).
//
// Launch shape, that of k_gc_pure_vle: one row per lane, 128-thread workgroups, the table, the lanes' row bytes and bond
// diameters in LDS, rows in the caller's class order or bucketed by class inside the workgroup.  The row pick is the last
// place where a lane waits for another.
//
// Registers (compiler's resource report, gfx950).  Left to itself the compiler gives the T2 evaluation of stage 2 AGPRs on top of
// the solver's 248 VGPRs -- 248 + 16 (inlined evaluation, 608 B scratch) or 248 + 32 (called, 772 B) -- and the kernel drops to
// ONE wave per SIMD for the sake of one evaluation per row, while the ~30-100 line evaluations of stage 1 are what a row pays.
// amdgpu_waves_per_eu(2) holds it to the 256 registers of k_gc_pure_vle: 248 VGPRs, no AGPRs, two waves per SIMD, 676 B of
// scratch per lane with the inlined evaluation (900 B with the call), against k_gc_pure_vle's 528 B.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pcsaft_hip.h"
#include "abi_common.hpp"
#include "block_order.hpp"
#include "gc_model.hpp"
#include "gc_kernel_common.hpp"
#include "gc_henry.hpp"

using namespace pcs;
using namespace pcs_abi;

namespace {

constexpr int GHBLOCK = 128;

__global__ __attribute__((amdgpu_waves_per_eu(2))) __launch_bounds__(GHBLOCK) void k_gc_henry(
    int solute, const double* __restrict__ table, int S, const unsigned char* __restrict__ rows, const double* __restrict__ phi,
    const double* __restrict__ temp, int64_t n, double* __restrict__ h, double* __restrict__ rho_vl, double* __restrict__ p_sat,
    double* __restrict__ dlnh_drho, double* __restrict__ dpdrho_l, uint8_t* __restrict__ status, int32_t* __restrict__ iters,
    const int32_t* __restrict__ order) {
    extern __shared__ double lds[];
    GcTable tb = stage_table(table, S, lds);
    double* bonds = lds + gc_table_doubles(S);          // [2*MAXE][GHBLOCK]: the bond diameters d_ab
    double* row_area = bonds + 2 * GC_MAXE * GHBLOCK;   // the lanes' row bytes (stage_row)
    const int t = threadIdx.x;
    const int64_t i = gc_pick_row<GHBLOCK>(rows, tb, n, order);
    if (i >= n) return;  // (behind every barrier of the kernel)
    const double T = temp[i];
    const double ph0 = phi[2 * i], ph1 = phi[2 * i + 1];
    SatResult r;
    r.p_star = r.rho_v = r.rho_l = r.dp_v = r.dp_l = 0.0;
    double hv = 0.0, dl = 0.0;
    int evals = 0;
    bool ok = is_finite_bits(T) && T > 0.0 && is_finite_bits(ph0) && is_finite_bits(ph1);
    if (ok) {  // lane-private from here on: an invalid row takes no part in any solve and no lane waits for it
        const unsigned char* row = stage_row(rows + (size_t)i * GC_ROW_BYTES, row_area);
        GcModelT<double> m;
        m.c.bond_dab = bonds + t;
        m.c.stride = GHBLOCK;
        gc_coef<double>(m.c, row, tb, ph0, ph1, T);
        ok = gc_henry_solvent(m, 1 - solute, r, evals);
        const double p = r.p_star * T * P_UNIT;
        ok = ok && is_finite_bits(p) && p > 0.0 && is_finite_bits(r.rho_v) && is_finite_bits(r.rho_l) && is_finite_bits(r.dp_v) &&
             is_finite_bits(r.dp_l);
        r.p_star = p;
        if (ok) {
            double mu_s, dmu;
            gc_henry_solute(m, solute, r.rho_l, mu_s, dmu);
            evals++;
            hv = (r.rho_l * T * P_UNIT) * exp(mu_s);
            dl = 1.0 / r.rho_l + dmu;
            ok = is_finite_bits(hv) && hv > 0.0 && is_finite_bits(dl);
        }
    }
    h[i] = ok ? hv : 0.0;
    if (rho_vl) {
        rho_vl[2 * i] = ok ? r.rho_v : 0.0;
        rho_vl[2 * i + 1] = ok ? r.rho_l : 0.0;
    }
    if (p_sat) p_sat[i] = ok ? r.p_star : 0.0;
    if (dlnh_drho) dlnh_drho[i] = ok ? dl : 0.0;
    if (dpdrho_l) dpdrho_l[i] = ok ? r.dp_l : 0.0;
    if (iters) iters[i] = ok ? evals : -1;
    status[i] = ok ? 0 : 1;
}

}  // namespace

extern "C" {

int pcs_gc_henry(int solute, const double* table, int S, const uint8_t* rows, const double* phi, const double* temp, int64_t n,
                 double* h, double* rho_vl, double* p_sat, double* dlnh_drho, double* dpdrho_l, uint8_t* status, int32_t* iters,
                 const int32_t* order, void* stream) {
    if (int e = gc_enter(S, n, table && rows && phi && temp && h && status, "pcs_gc_henry: null required pointer"); e != GO_ON)
        return e;
    if (solute != 0 && solute != 1) return fail_msg("pcs_gc_henry", "solute must be 0 or 1 (molecule index)");
    if (int e = aligned16("pcs_gc_henry", "rows", rows)) return e;
    const size_t lds = gc_lds_bytes(S, GHBLOCK, 2 * GC_MAXE + GC_ROW_LDS_DOUBLES);
    hipLaunchKernelGGL(k_gc_henry, dim3(grid_for(n, GHBLOCK)), dim3(GHBLOCK), lds, as_stream(stream), solute, table, S, rows, phi,
                       temp, n, h, rho_vl, p_sat, dlnh_drho, dpdrho_l, status, iters, order);
    return launched("k_gc_henry launch");
}

}  // extern "C"
