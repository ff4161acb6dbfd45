// Gradients of the gc bubble / dew pressure AND of the incipient-phase mole fraction at a converged bubble / dew point w.r.t.
// the six dispersion aggregates and T (see include/pcsaft_hip.h: pcs_gc_jacobian, pcs_gc_point_jacobian; the mathematics is
// mix_jacobian.hpp's and mix_incipient.hpp's).  Own translation unit, compiled with the flags of gc_kernels.hip
// (feos_torch_amd/build.py, GUARDED_SOURCES).  One kernel template is the per-row backward pass of every GcPcSaftMix bubble / dew
// call: pcs_gc_jacobian (the default calls) launches <true, false>, pcs_gc_point_jacobian (incipient_molefracs=True) the
// instantiation for the blocks it is asked for.
//
// State and equations: u = (ln rho_spec, ln rho_inc_0, ln rho_inc_1), F = (mu_0^S - mu_0^I, mu_1^S - mu_1^I, p^S - p^I) = 0,
// J = dF/du, J^T w = dp^vap/du (implicit-function form).  k_ab and phi enter the model only through the aggregates
// (feos_torch/gc_pcsaft.py:181-194), the host chains them (gc_pcsaft.py in this package).  y0 = rho_inc_0 / (rho_inc_0 +
// rho_inc_1) has no explicit dependence on theta:
//     J^T w_y = dy0/du = (0, y0 y1, -y0 y1),    dy0/dtheta = -w_y . dF/dtheta|_u
// without a unit factor and without the p_red term of the temperature column.  One coefficient set, two phase evaluations, one
// elimination with two right-hand sides (solve3_pair), one dual direction (T) contracted once per requested functional.
// The bits of the pressure block (jac_p, agg) are pinned, row by row, by tests/golden/gc_jacobian_bits.json
// (tests/test_gc_jacobian_bits_gpu.py), in every instantiation that writes it.  For that the template is instantiated per set
// of requested blocks, so that the pressure block's statements stand unguarded; the composition block follows in statements of
// its own that read the phase derivatives through `detached` copies.  Both matter for the bits of jac_p: this unit is compiled
// with -fassociative-math, and a subexpression shared between the blocks, or a branch around the pressure block, moved its
// rounding (measured: up to 1.3e-13 relative on 40 % of the entries).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pcsaft_hip.h"
#include "abi_common.hpp"
#include "gc_model.hpp"
#include "gc_kernel_common.hpp"
#include "mix_solver.hpp"
#include "mix_incipient.hpp"  // solve3_pair

using namespace pcs;
using namespace pcs_abi;

namespace {

// 59 doubles of LDS per thread (bond diameters of the double and the dual model, row bytes); a 256-thread workgroup shares ONE
// copy of the table among four waves (S = 22: 131 KB, S = 32: 144 KB of the CU's 160 KB) -- 64-thread workgroups fit three times
// (one wave each): the kernel holds a full register file per wave, so resident waves per CU are what counts
constexpr int GPJBLOCK = 256;
constexpr int GC_DIRS = 7;   // A00, A01, A11, B00, B01, B11, T
constexpr int GC_CHUNK = 1;  // the only dual-number direction is T

// A copy of x the compiler cannot identify with x (no instruction).  The composition block reads the phase derivatives through
// it: shared with the pressure block as common subexpressions they would end the pressure block's expression trees at other
// places than in <true, false>, and under -fassociative-math the pressure columns would leave their pinned bits.
__device__ __forceinline__ double detached(double x) {
    asm volatile("" : "+v"(x));
    return x;
}

// WANT_P / WANT_Y: which blocks are written (the other pointer is not touched)
template <bool WANT_P, bool WANT_Y>
__global__ __launch_bounds__(GPJBLOCK) void k_gc_point_jacobian(int dew, const double* __restrict__ table, int S,
                                                                const unsigned char* __restrict__ rows,
                                                                const double* __restrict__ phi,
                                                                const double* __restrict__ temp,
                                                                const double* __restrict__ rho4, int64_t n,
                                                                double* __restrict__ jac_p, double* __restrict__ jac_y,
                                                                double* __restrict__ agg, const int32_t* __restrict__ order) {
    typedef DN<double, GC_CHUNK> G;
    typedef T1<G> R;
    extern __shared__ double lds[];
    GcTable tb = stage_table(table, S, lds);
    double* bonds = lds + gc_table_doubles(S);                         // double model: [2*MAXE dab] x block
    G* gbonds = reinterpret_cast<G*>(bonds + 2 * GC_MAXE * GPJBLOCK);  // dual model dab
    int64_t i = (int64_t)blockIdx.x * GPJBLOCK + threadIdx.x;
    if (i >= n) return;
    if (order) {  // class order of the rows (see pcs_gc_bubble_dew)
        i = order[i];
        if (i < 0 || i >= n) return;
    }
    // (row bytes staged behind the dual model's bond area)
    const unsigned char* row = stage_row(rows + (size_t)i * GC_ROW_BYTES, bonds + (2 * GC_MAXE + 2 * GC_MAXE * (1 + GC_CHUNK)) * GPJBLOCK);
    const double T = temp[i], ph0 = phi[2 * i], ph1 = phi[2 * i + 1];
    const double4 r4 = reinterpret_cast<const double4*>(rho4)[i];  // (V0, V1, L0, L1)
    const double s0 = dew ? r4.x : r4.z, s1 = dew ? r4.y : r4.w, i0 = dew ? r4.z : r4.x, i1 = dew ? r4.w : r4.y;
    GcModelT<double> m;
    m.c.bond_dab = bonds + threadIdx.x;
    m.c.stride = GPJBLOCK;
    gc_coef<double>(m.c, row, tb, ph0, ph1, T);
    if (agg) {
#pragma unroll
        for (int k = 0; k < 3; k++) { agg[6 * i + k] = m.c.A[k]; agg[6 * i + 3 + k] = m.c.B[k]; }
    }
    PhaseEval s = phase_eval(m, s0, s1);
    PhaseEval nn = phase_eval(m, i0, i1);
    const double rs = s0 + s1, z0 = s0 / rs, z1 = s1 / rs;
    const double ri = i0 + i1, y0 = i0 / ri, y1 = i1 / ri;
    double J[3][3];
    J[0][0] = rs * (z0 * (1.0 / s.r0 + s.h00) + z1 * s.h01);
    J[1][0] = rs * (z0 * s.h01 + z1 * (1.0 / s.r1 + s.h11));
    J[2][0] = rs * (z0 * s.dp0() + z1 * s.dp1());
    J[0][1] = -i0 * (1.0 / i0 + nn.h00);
    J[1][1] = -i0 * nn.h01;
    J[2][1] = -i0 * nn.dp0();
    J[0][2] = -i1 * nn.h01;
    J[1][2] = -i1 * (1.0 / i1 + nn.h11);
    J[2][2] = -i1 * nn.dp1();
    // J^T and the right-hand sides: dp^vap/du and, when the composition is asked for, dy0/du
    double A[3][5];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int cc = 0; cc < 3; cc++) A[r][cc] = J[cc][r];
        A[r][3] = 0.0;
    }
    if (dew) {
        A[0][3] = J[2][0];
    } else {
        A[1][3] = -J[2][1];
        A[2][3] = -J[2][2];
    }
    A[0][4] = 0.0;
    A[1][4] = y0 * y1;
    A[2][4] = -(y0 * y1);
    double w[3], wy[3];
    const bool ok = solve3_pair(A, w, wy);
    const double p_red = dew ? s.p() : nn.p();
    const double nanv = __longlong_as_double(0x7ff8000000000000LL);
    double* g = jac_p + GC_DIRS * i;
    double* gy = jac_y + GC_DIRS * i;

    // (1) the six aggregates: the dispersion term is linear in them, a_disp = F1 sum_k A_k q_k + F2 sum_k B_k q_k with
    //     q = (r0^2, r0 r1, r1^2): d(a, da/dr0, da/dr1)/dA_k = (F1 q_k, dF1/dr0 q_k + F1 dq_k/dr0, ...) -- no dual pass.  The
    //     composition block follows in statements of its own on detached copies (see `detached`): y0 has no explicit term
    {
        typedef T1<double> Q;
        Q F1s, F2s, F1i, F2i;
        dispersion_factors(m.c, Q(s0, 1.0, 0.0), Q(s1, 0.0, 1.0), F1s, F2s);
        dispersion_factors(m.c, Q(i0, 1.0, 0.0), Q(i1, 0.0, 1.0), F1i, F2i);
        if constexpr (WANT_P) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                // q_k and its gradient in both phases
                const double qs = (k == 0) ? s0 * s0 : (k == 1 ? s0 * s1 : s1 * s1);
                const double qs0 = (k == 0) ? 2.0 * s0 : (k == 1 ? s1 : 0.0), qs1 = (k == 0) ? 0.0 : (k == 1 ? s0 : 2.0 * s1);
                const double qi = (k == 0) ? i0 * i0 : (k == 1 ? i0 * i1 : i1 * i1);
                const double qi0 = (k == 0) ? 2.0 * i0 : (k == 1 ? i1 : 0.0), qi1 = (k == 0) ? 0.0 : (k == 1 ? i0 : 2.0 * i1);
#pragma unroll
                for (int ab = 0; ab < 2; ab++) {
                    const Q& Fs = ab == 0 ? F1s : F2s;
                    const Q& Fi = ab == 0 ? F1i : F2i;
                    const double aS = Fs.v * qs, gS0 = Fs.g0 * qs + Fs.v * qs0, gS1 = Fs.g1 * qs + Fs.v * qs1;
                    const double aI = Fi.v * qi, gI0 = Fi.g0 * qi + Fi.v * qi0, gI1 = Fi.g1 * qi + Fi.v * qi1;
                    const double dF0 = gS0 - gI0, dF1 = gS1 - gI1;
                    const double dpS = -aS + s0 * gS0 + s1 * gS1;
                    const double dpI = -aI + i0 * gI0 + i1 * gI1;
                    const double dp = (dew ? dpS : dpI) - (w[0] * dF0 + w[1] * dF1 + w[2] * (dpS - dpI));
                    g[3 * ab + k] = ok ? dp * T * P_UNIT : nanv;
                }
            }
        }
        if constexpr (WANT_Y) {
            const double t0 = detached(s0), t1 = detached(s1), j0 = detached(i0), j1 = detached(i1);
#pragma unroll
            for (int ab = 0; ab < 2; ab++) {
                const Q& Fs = ab == 0 ? F1s : F2s;
                const Q& Fi = ab == 0 ? F1i : F2i;
                const double fsv = detached(Fs.v), fs0 = detached(Fs.g0), fs1 = detached(Fs.g1);
                const double fiv = detached(Fi.v), fi0 = detached(Fi.g0), fi1 = detached(Fi.g1);
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const double qs = (k == 0) ? t0 * t0 : (k == 1 ? t0 * t1 : t1 * t1);
                    const double qs0 = (k == 0) ? 2.0 * t0 : (k == 1 ? t1 : 0.0), qs1 = (k == 0) ? 0.0 : (k == 1 ? t0 : 2.0 * t1);
                    const double qi = (k == 0) ? j0 * j0 : (k == 1 ? j0 * j1 : j1 * j1);
                    const double qi0 = (k == 0) ? 2.0 * j0 : (k == 1 ? j1 : 0.0), qi1 = (k == 0) ? 0.0 : (k == 1 ? j0 : 2.0 * j1);
                    const double aS = fsv * qs, gS0 = fs0 * qs + fsv * qs0, gS1 = fs1 * qs + fsv * qs1;
                    const double aI = fiv * qi, gI0 = fi0 * qi + fiv * qi0, gI1 = fi1 * qi + fiv * qi1;
                    const double dpS = -aS + t0 * gS0 + t1 * gS1;
                    const double dpI = -aI + j0 * gI0 + j1 * gI1;
                    const double dy = -(wy[0] * (gS0 - gI0) + wy[1] * (gS1 - gI1) + wy[2] * (dpS - dpI));
                    gy[3 * ab + k] = ok ? dy : nanv;
                }
            }
        }
    }

    // (2) T: one dual-number direction, both phases through one evaluation site, contracted once per requested functional
    {
        G gT;
        gT.v = T;
        gT.e[0] = 1.0;
        GcCoef<G> c;
        c.bond_dab = gbonds + threadIdx.x;
        c.bond_cnt = m.c.bond_cnt;  // counts are shared (written identically)
        c.stride = GPJBLOCK;
        gc_coef<G>(c, row, tb, ph0, ph1, gT);
        double av[2], ag0[2], ag1[2];
#pragma unroll 1
        for (int ph = 0; ph < 2; ph++) {
            const double q0 = ph == 0 ? s0 : i0, q1 = ph == 0 ? s1 : i1;
            R a = gc_a_tangent<G, R>(c, R(G(q0), G(1.0), G(0.0)), R(G(q1), G(0.0), G(1.0)));
            if (ph == 0) { av[0] = a.v.e[0]; ag0[0] = a.g0.e[0]; ag1[0] = a.g1.e[0]; }
            else { av[1] = a.v.e[0]; ag0[1] = a.g0.e[0]; ag1[1] = a.g1.e[0]; }
        }
        if constexpr (WANT_P) {
            const double dF0 = ag0[0] - ag0[1], dF1 = ag1[0] - ag1[1];
            const double dpS = -av[0] + s0 * ag0[0] + s1 * ag1[0];
            const double dpI = -av[1] + i0 * ag0[1] + i1 * ag1[1];
            const double dp = (dew ? dpS : dpI) - (w[0] * dF0 + w[1] * dF1 + w[2] * (dpS - dpI));
            g[6] = ok ? dp * T * P_UNIT + p_red * P_UNIT : nanv;
        }
        if constexpr (WANT_Y) {
            const double t0 = detached(s0), t1 = detached(s1), j0 = detached(i0), j1 = detached(i1);
            const double vS = detached(av[0]), vI = detached(av[1]);
            const double gS0 = detached(ag0[0]), gI0 = detached(ag0[1]), gS1 = detached(ag1[0]), gI1 = detached(ag1[1]);
            const double dpS = -vS + t0 * gS0 + t1 * gS1;
            const double dpI = -vI + j0 * gI0 + j1 * gI1;
            const double dy = -(wy[0] * (gS0 - gI0) + wy[1] * (gS1 - gI1) + wy[2] * (dpS - dpI));
            gy[6] = ok ? dy : nanv;
        }
    }
}

// The one launch behind both entry points.  jac_y = nullptr, as pcs_gc_jacobian passes it, selects <true, false>
int launch_gc_point_jacobian(int dew, const double* table, int S, const uint8_t* rows, const double* phi, const double* temp,
                             const double* rho4, int64_t n, double* jac_p, double* jac_y, double* agg, const int32_t* order,
                             void* stream) {
    const unsigned grid = grid_for(n, GPJBLOCK);
    // double model: 2*MAXE doubles per thread; dual model dab: 2*MAXE * (1 + GC_CHUNK) doubles per thread; the row bytes
    const size_t lds = gc_lds_bytes(S, GPJBLOCK, 2 * GC_MAXE + 2 * GC_MAXE * (1 + GC_CHUNK) + GC_ROW_LDS_DOUBLES);
    auto launch = [&](auto kernel) -> int {
        if (lds > 64 * 1024) {  // above the default dynamic-LDS limit
            hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (ea != hipSuccess) return fail("k_gc_point_jacobian attribute", ea);
        }
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(GPJBLOCK), lds, as_stream(stream), dew, table, S, rows, phi, temp, rho4, n, jac_p,
                           jac_y, agg, order);
        return 0;
    };
    if (int e = jac_p && jac_y ? launch(k_gc_point_jacobian<true, true>) : jac_p ? launch(k_gc_point_jacobian<true, false>)
                                                                                  : launch(k_gc_point_jacobian<false, true>))
        return e;
    return launched("k_gc_point_jacobian launch");
}

}  // namespace

extern "C" {

int pcs_gc_jacobian(int dew, const double* table, int S, const uint8_t* rows, const double* phi, const double* temp,
                    const double* rho4, int64_t n, double* jac, double* agg, const int32_t* order, void* stream) {
    if (int e = gc_enter(S, n, table && rows && phi && temp && rho4 && jac, "pcs_gc_jacobian: null required pointer"); e != GO_ON) return e;
    if (int e = aligned16("pcs_gc_jacobian", "rows", rows)) return e;
    return launch_gc_point_jacobian(dew, table, S, rows, phi, temp, rho4, n, jac, nullptr, agg, order, stream);
}

int pcs_gc_point_jacobian(int dew, const double* table, int S, const uint8_t* rows, const double* phi, const double* temp,
                          const double* rho4, int64_t n, double* jac_p, double* jac_y, double* agg, const int32_t* order,
                          void* stream) {
    g_err[0] = 0;
    if (check_n(n)) return fail_msg("pcs_gc_point_jacobian", "n must be in [0, 2^31) rows per call (shard larger batches)");
    if (S < 1 || S > GC_MAXS) return fail_msg("pcs_gc_point_jacobian", "S, the number of segment types, must be in [1, 32]");
    if (n == 0) return 0;
    if (!table || !rows || !phi || !temp || !rho4)
        return fail_msg("pcs_gc_point_jacobian", "null required pointer (table, rows, phi, temp, rho4)");
    if (!jac_p && !jac_y) return fail_msg("pcs_gc_point_jacobian", "jac_p and jac_y are both null (one output is required)");
    if (int e = aligned16("pcs_gc_point_jacobian", "rows", rows)) return e;
    return launch_gc_point_jacobian(dew, table, S, rows, phi, temp, rho4, n, jac_p, jac_y, agg, order, stream);
}

}  // extern "C"
