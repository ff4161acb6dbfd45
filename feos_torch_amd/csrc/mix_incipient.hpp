// Gradients of TWO functionals of a converged binary bubble / dew point (device only): the pressure, as mix_jacobian.hpp,
// and the mole fraction of component 1 in the INCIPIENT phase (vapour for bubble, liquid for dew),
//     y0 = rho_inc_0 / (rho_inc_0 + rho_inc_1),
// w.r.t. (16 component parameters, k_ij, eps_AiBj, T).  Same state and equations as mix_jacobian.hpp:
//     u = (ln rho_spec, ln rho_inc_0, ln rho_inc_1),   F(u, theta) = (mu_0^S - mu_0^I, mu_1^S - mu_1^I, p^S - p^I) = 0.
// Unlike the pressure, y0 has no explicit dependence on theta and is not stationary in u: its whole gradient is the
// response of the densities,
//     dy0/du = (0, y0 y1, -y0 y1),    J^T w = dy0/du,    dy0/dtheta = -w . dF/dtheta|_u.
// With p^X = -a^X + rho^X . grad a^X and F_i = grad_i a^S - grad_i a^I this is again one scalar alpha a + beta . grad a per
// phase (the form mix_a_adjoint consumes):
//     specified phase:  alpha =  w2,  beta = -w2 rho^S - (w0, w1)
//     incipient phase:  alpha = -w2,  beta =  w2 rho^I + (w0, w1)
// and dy0/dtheta = sum_k abar_k dc_k/dtheta (mix_coef_gradient) without any unit factor: y0 is dimensionless, and the
// temperature column has no p/T term.
// Both functionals share the coefficient set, the two phase evaluations and the elimination of J^T (solve3 of
// mix_solver.hpp carries one right-hand side; solve3_pair below is the same elimination with two).  The adjoint block is
// used twice in sequence -- zero, accumulate both phases, contract, write -- once per requested functional.
#pragma once
#include "mix_jacobian.hpp"

namespace pcs {

// solve3 (mix_solver.hpp) with two right-hand sides: A[r][3] -> x, A[r][4] -> y.  Same pivoting, same operations per column.
PCS_DEV void swap_rows5(double* a, double* b) {
#pragma unroll
    for (int j = 0; j < 5; j++) { double t = a[j]; a[j] = b[j]; b[j] = t; }
}
PCS_DEV bool solve3_pair(double A[3][5], double* x, double* y) {
    if (fabs(A[1][0]) > fabs(A[0][0])) swap_rows5(A[0], A[1]);
    if (fabs(A[2][0]) > fabs(A[0][0])) swap_rows5(A[0], A[2]);
    if (A[0][0] == 0.0) return false;
    const double inv = d_recip(A[0][0]);
    const double f1 = A[1][0] * inv, f2 = A[2][0] * inv;
#pragma unroll
    for (int j = 1; j < 5; j++) { A[1][j] -= f1 * A[0][j]; A[2][j] -= f2 * A[0][j]; }
    if (fabs(A[2][1]) > fabs(A[1][1])) swap_rows5(A[1], A[2]);
    if (A[1][1] == 0.0) return false;
    const double inv1 = d_recip(A[1][1]);
    const double f = A[2][1] * inv1;
    A[2][2] -= f * A[1][2];
    A[2][3] -= f * A[1][3];
    A[2][4] -= f * A[1][4];
    if (A[2][2] == 0.0) return false;
    const double inv2 = d_recip(A[2][2]);
    x[2] = A[2][3] * inv2;
    x[1] = (A[1][3] - A[1][2] * x[2]) * inv1;
    x[0] = (A[0][3] - A[0][1] * x[1] - A[0][2] * x[2]) * inv;
    y[2] = A[2][4] * inv2;
    y[1] = (A[1][4] - A[1][2] * y[2]) * inv1;
    y[0] = (A[0][4] - A[0][1] * y[1] - A[0][2] * y[2]) * inv;
    return true;
}

// spec = (rho_spec_0, rho_spec_1), inc = (rho_inc_0, rho_inc_1).  gp[19] in Pa per unit of theta (as mix_jacobian), gy[19]
// per unit of theta; either may be null.  adj: lane-strided scratch of ADJ_SLOTS doubles, used once per functional.
PCS_DEV void mix_point_jacobian(const double par[16], double k0, double k1, double T, double s0, double s1, double i0,
                                double i1, bool spec_is_vapor, double* __restrict__ gp, double* __restrict__ gy, double* adj,
                                int adj_stride) {
    MixModelD m;
    mix_coef<double>(m.c, par, k0, k1, T);
    const PhaseEval s = phase_eval(m, s0, s1);
    const PhaseEval n = phase_eval(m, i0, i1);
    const double rs = s0 + s1, z0 = s0 / rs, z1 = s1 / rs;
    const double ri = i0 + i1, y0 = i0 / ri, y1 = i1 / ri;
    // J[equation][unknown] as in mix_jacobian; the augmented matrix holds J^T and the two right-hand sides
    double J[3][3];
    J[0][0] = rs * (z0 * (1.0 / s.r0 + s.h00) + z1 * s.h01);
    J[1][0] = rs * (z0 * s.h01 + z1 * (1.0 / s.r1 + s.h11));
    J[2][0] = rs * (z0 * s.dp0() + z1 * s.dp1());
    J[0][1] = -i0 * (1.0 / i0 + n.h00);
    J[1][1] = -i0 * n.h01;
    J[2][1] = -i0 * n.dp0();
    J[0][2] = -i1 * n.h01;
    J[1][2] = -i1 * (1.0 / i1 + n.h11);
    J[2][2] = -i1 * n.dp1();
    double A[3][5];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int cc = 0; cc < 3; cc++) A[r][cc] = J[cc][r];  // J^T
        A[r][3] = 0.0;
    }
    if (spec_is_vapor) {
        A[0][3] = J[2][0];  // dp^S/du
    } else {
        A[1][3] = -J[2][1];  // dp^I/du
        A[2][3] = -J[2][2];
    }
    A[0][4] = 0.0;  // dy0/du
    A[1][4] = y0 * y1;
    A[2][4] = -(y0 * y1);
    double wp[3], wy[3];
    const bool ok = solve3_pair(A, wp, wy);
    const double p_red = spec_is_vapor ? s.p() : n.p();
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll 1
    for (int f = 0; f < 2; f++) {
        double* __restrict__ g = f == 0 ? gp : gy;
        if (!g) continue;  // kernel argument: uniform over the launch
        // (alpha, beta) of the two phases: [0] specified, [1] incipient
        double alpha[2], beta0[2], beta1[2];
        if (f == 0) {  // the pressure, taken on the vapour phase: mix_jacobian
            if (spec_is_vapor) {
                const double u = 1.0 - wp[2];
                alpha[0] = -u;      beta0[0] = u * s0 - wp[0];      beta1[0] = u * s1 - wp[1];
                alpha[1] = -wp[2];  beta0[1] = wp[2] * i0 + wp[0];  beta1[1] = wp[2] * i1 + wp[1];
            } else {
                const double u = 1.0 + wp[2];
                alpha[0] = wp[2];   beta0[0] = -wp[2] * s0 - wp[0]; beta1[0] = -wp[2] * s1 - wp[1];
                alpha[1] = -u;      beta0[1] = u * i0 + wp[0];      beta1[1] = u * i1 + wp[1];
            }
        } else {  // y0: -w . dF/dtheta only
            alpha[0] = wy[2];   beta0[0] = -wy[2] * s0 - wy[0]; beta1[0] = -wy[2] * s1 - wy[1];
            alpha[1] = -wy[2];  beta0[1] = wy[2] * i0 + wy[0];  beta1[1] = wy[2] * i1 + wy[1];
        }
#pragma unroll
        for (int k = 0; k < ADJ_SLOTS; k++) adj[k * adj_stride] = 0.0;
#pragma unroll 1
        for (int ph = 0; ph < 2; ph++) {
            const double q0 = ph == 0 ? s0 : i0, q1 = ph == 0 ? s1 : i1;
            const double al = ph == 0 ? alpha[0] : alpha[1], b0 = ph == 0 ? beta0[0] : beta0[1], b1 = ph == 0 ? beta1[0] : beta1[1];
            mix_a_adjoint(m.c, q0, q1, b0, b1, al, adj, adj_stride);
        }
        double e[MIX_DIRS];
        mix_coef_gradient(par, k0, k1, T, adj, adj_stride, e);
        const double unit = f == 0 ? T * P_UNIT : 1.0;             // p [Pa] = p_red T kB/A^3; y0 has no unit
        const double explicit_T = f == 0 ? p_red * P_UNIT : 0.0;  // dp/dT at fixed p_red
#pragma unroll
        for (int d = 0; d < MIX_DIRS; d++) {
            double val = e[d] * unit;
            if (d == 18) val += explicit_T;
            if (!ok) val = nan;
            g[d] = val;
        }
    }
}

}  // namespace pcs
