// fp32 pre-solve of the pure-component VLE (device only).
//
// On gfx950 an fp32 VALU op issues in half the cycles of an fp64 one and 1/x, log, sqrt are single
// (quarter-rate) instructions instead of ~5 / ~45 / ~20-instruction fp64 sequences, so one fp32
// evaluation of a(rho), a', a'' costs ~0.35 of the fp64 one.  Newton's method is self-correcting:
// the zero-pressure liquid root, the ideal-gas vapour estimate and the first coupled iterations
// are therefore run in fp32 down to its noise floor (~1e-6 relative), and the fp64 iteration of
// pure_solver.hpp starts from that point and needs 1-2 iterations instead of 4-5 + initialiser.
// The result is defined by the fp64 iterations alone; a lane whose fp32 pass leaves the
// representable range or misbehaves simply takes the all-fp64 path.
#pragma once
#include "pure_model.hpp"

namespace pcs {

constexpr float PCS_F32_TAYLOR_MAX = 1e-3f;
constexpr float PCS_F32_PREDICT_TOL_L = 5e-6f;
constexpr float PCS_F32_PREDICT_TOL_V = 5e-5f;
constexpr float PCS_F32_PREDICT_CMAX = 1e3f;
constexpr int PCS_F32_DENSE_LEVELS = 3;  // rungs of the fp32 liquid root's dense-side ladder (1 = eta 0.58 only)
// Lean coupled iterations (a and a' only; dp/drho carried and updated from the pressures in hand: carry_slope,
// presolve_coupled):
// LEAN_MAX:   largest relative vapour step after which the next vapour evaluation may be lean: every ordinary step (a step
//             taken in ln(rho) always forces the full form).  It does not bound the error of the slope handed to the fp64
//             finish.  That slope comes from the lane's last update: trapezoid across a step d, error p''' d^2 / 12 -- small
//             for the near-quadratic p(rho) of a vapour even at a large d -- or three-point, ~ p''' d0 d1 / 6.  No a-priori
//             bound is claimed for it; it was measured instead: the CPU restatement of the iteration puts it at 1.2e-3 at
//             most (median 3e-5), and p_sat against the long-double oracle on 1e6 rows is no worse than with the
//             exact slopes of the full evaluation.
// SECANT_MIN: the pressure carries ~1e-7 rho (1 + |a'|) of fp32 rounding noise, the quotient is taken over step * rho and
//             doubled by the trapezoid: its relative error is ~2e-7 (1 + |a'|) / (step p').  Updated only when that is
//             below ~1e-3, i.e. step * p' >= 3e-4 (1 + |a'|); below it the kept slope is off by less than that anyway.
constexpr float PCS_F32_LEAN_MAX = 0.5f;
constexpr float PCS_F32_SECANT_MIN = 3e-4f;
constexpr float PCS_F32_LIQ_TOL = 1e-1f;  // relative (scaled-Newton) step at which the fp32 liquid initialiser hands over to the coupled iteration

struct F2 {  // value, d/drho, d2/drho2 in fp32
    float v, d1, d2;
};
PCS_DEV F2 f2(float v, float d1, float d2) { F2 r; r.v = v; r.d1 = d1; r.d2 = d2; return r; }
PCS_DEV F2 operator+(F2 a, F2 b) { return f2(a.v + b.v, a.d1 + b.d1, a.d2 + b.d2); }
PCS_DEV F2 operator-(F2 a, F2 b) { return f2(a.v - b.v, a.d1 - b.d1, a.d2 - b.d2); }
PCS_DEV F2 operator+(F2 a, float b) { return f2(a.v + b, a.d1, a.d2); }
PCS_DEV F2 operator-(float b, F2 a) { return f2(b - a.v, -a.d1, -a.d2); }
PCS_DEV F2 operator*(F2 a, float b) { return f2(a.v * b, a.d1 * b, a.d2 * b); }
PCS_DEV F2 operator*(F2 a, F2 b) {
    return f2(a.v * b.v, fmaf(a.d1, b.v, a.v * b.d1), fmaf(a.d2, b.v, fmaf(2.0f * a.d1, b.d1, a.v * b.d2)));
}
PCS_DEV F2 chainf(F2 a, float f0, float f1, float f2_) { return f2(f0, f1 * a.d1, fmaf(f2_, a.d1 * a.d1, f1 * a.d2)); }
// raw v_log_f32 / v_exp_f32 (the library __logf / __expf wrap them in a denormal rescue: v_cmp + v_cndmask + v_ldexp,
// ~5 VALU each).  Arguments here are normal fp32 numbers or the lane falls back to the fp64 path (non-finite result).
PCS_DEV float f_log(float x) { return __builtin_amdgcn_logf(x) * 0.69314718f; }
PCS_DEV float f_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504f); }
PCS_DEV F2 recipf(F2 a) {
    float r = __builtin_amdgcn_rcpf(a.v);
    float r2 = r * r;
    return chainf(a, r, -r2, 2.0f * r2 * r);
}
PCS_DEV F2 logf2(F2 a) {
    float r = __builtin_amdgcn_rcpf(a.v);
    return chainf(a, f_log(a.v), r, -r * r);
}
PCS_DEV F2 sqrtf2(F2 a) {
    float s = __builtin_amdgcn_sqrtf(a.v);
    float h = 0.5f * __builtin_amdgcn_rcpf(s);
    return chainf(a, s, h, -0.5f * h * __builtin_amdgcn_rcpf(a.v));
}
template <int N>
PCS_DEV F2 hornerf(const float* coef, F2 x) {  // x.d2 == 0 (x = eta = ceta * rho)
    float p = coef[N - 1], d1 = 0.0f, d2 = 0.0f;
#pragma unroll
    for (int i = N - 2; i >= 0; i--) {
        d2 = fmaf(d2, x.v, d1);
        d1 = fmaf(d1, x.v, p);
        p = fmaf(p, x.v, coef[i]);
    }
    return f2(p, d1 * x.d1, 2.0f * d2 * (x.d1 * x.d1));
}

struct F1 {  // value, d/drho in fp32: the dipole arithmetic of the evaluation without a''
    float v, d1;
};
PCS_DEV F1 f1(float v, float d1) { F1 r; r.v = v; r.d1 = d1; return r; }
PCS_DEV F1 operator-(F1 a, F1 b) { return f1(a.v - b.v, a.d1 - b.d1); }
PCS_DEV F1 operator*(F1 a, float b) { return f1(a.v * b, a.d1 * b); }
PCS_DEV F1 operator*(F1 a, F1 b) { return f1(a.v * b.v, fmaf(a.d1, b.v, a.v * b.d1)); }
PCS_DEV F1 recipf(F1 a) {
    float r = __builtin_amdgcn_rcpf(a.v);
    return f1(r, -(r * r) * a.d1);
}
template <int N>
PCS_DEV F1 hornerf(const float* coef, F1 x) {
    float p = coef[N - 1], d1 = 0.0f;
#pragma unroll
    for (int i = N - 2; i >= 0; i--) {
        d1 = fmaf(d1, x.v, p);
        p = fmaf(p, x.v, coef[i]);
    }
    return f1(p, d1 * x.d1);
}

struct PureCoefF {
    float m, mm1, ceta, ai[7], bi[7], kd1, kd2, j1[5], j2[4], qm, da, na, nb;
    float m1, m2;  // (m-1)/m, (m-2)/m: ai[] / bi[] are linear in m1 and m1 m2 (read by pure_eval_start_f32 only)
    bool polar, assoc;
};

PCS_DEV void to_f32(const PureCoef<double>& c, PureCoefF& f) {
    f.m = (float)c.m; f.mm1 = (float)c.mm1; f.ceta = (float)c.ceta;
    const float rm = __builtin_amdgcn_rcpf(f.m);
    f.m1 = f.mm1 * rm; f.m2 = (f.m - 2.0f) * rm;
#pragma unroll
    for (int i = 0; i < 7; i++) { f.ai[i] = (float)c.ai[i]; f.bi[i] = (float)c.bi[i]; }
    f.kd1 = (float)c.kd1; f.kd2 = (float)c.kd2;
    f.polar = c.polar; f.assoc = c.assoc;
    if (c.polar) {
#pragma unroll
        for (int i = 0; i < 5; i++) f.j1[i] = (float)c.j1[i];
#pragma unroll
        for (int i = 0; i < 4; i++) f.j2[i] = (float)c.j2[i];
        f.qm = (float)c.qm;
    }
    f.da = (float)c.da; f.na = (float)c.na; f.nb = (float)c.nb;
}

// Native fp32 version of pure_coef() (pure_model.hpp): the pre-solve needs its coefficients to ~1e-6 only, and
// computing them from the fp32 parameters keeps the 33 fp64 coefficients out of the registers until the fp64
// finish needs them.
PCS_DEV void pure_coef_f32(PureCoefF& f, const double* par, double T64) {
    const float m = (float)par[0], sigma = (float)par[1], eps = (float)par[2], mu = (float)par[3];
    const float rT = __builtin_amdgcn_rcpf((float)T64);
    const float s3 = sigma * sigma * sigma;
    const float e = eps * rT;
    const float d = sigma * (1.0f - 0.12f * f_exp(-3.0f * e));
    f.m = m;
    f.mm1 = m - 1.0f;
    f.ceta = (float)FRAC_PI_6 * (m * (d * d * d));
    const float rm = __builtin_amdgcn_rcpf(m);
    const float m1 = f.mm1 * rm;
    const float m2 = (m - 2.0f) * rm;
    f.m1 = m1;
    f.m2 = m2;
#pragma unroll
    for (int i = 0; i < 7; i++) {
        f.ai[i] = fmaf(m1, fmaf(m2, (float)A2[i], (float)A1[i]), (float)A0[i]);
        f.bi[i] = fmaf(m1, fmaf(m2, (float)B2[i], (float)B1[i]), (float)B0[i]);
    }
    const float pref = (float)(-PI) * ((m * m) * (e * s3));
    f.kd1 = 2.0f * pref;
    f.kd2 = pref * (m * e);
    f.polar = mu != 0.0f;
    f.qm = 0.0f;
    if (f.polar) {
        const float mu2t = (mu * mu) * (rm * rT) * (float)MU2_UNIT;
        const bool clamp = m > 2.0f;
        const float md1 = clamp ? 0.5f : m1;
        const float md2 = clamp ? 0.0f : md1 * m2;
        const float rs3 = __builtin_amdgcn_rcpf(s3);
        const float f2c = (float)(-PI) * rs3;
        const float f3c = (float)(-PI_SQ_43) * (rs3 * mu2t);
#pragma unroll
        for (int i = 0; i < 5; i++) {
            float a = (float)AD[i][0] + md1 * (float)AD[i][1] + md2 * (float)AD[i][2];
            if (i < 3) a = a + ((float)BD[i][0] + md1 * (float)BD[i][1] + md2 * (float)BD[i][2]) * e;
            f.j1[i] = a * f2c;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) f.j2[i] = ((float)CD[i][0] + md1 * (float)CD[i][1] + md2 * (float)CD[i][2]) * f3c;
        f.qm = mu2t * mu2t;
    }
    f.na = (float)par[6];
    f.nb = (float)par[7];
    const bool sites = (f.na != 0.0f) || (f.nb != 0.0f);
    f.da = (f_exp((float)par[5] * rT) - 1.0f) * s3 * (float)par[4];
    f.assoc = sites && f.da != 0.0f;
}

struct EvalF { float a, p, dp, mu; };

// Hard sphere, hard chain and dispersion of a pure component are a = rho F(eta) + rho^2 G(eta), eta = ceta rho, with
//   F = m HS - (m-1) ln g,   HS = (4 eta - 3 eta^2) u^2,   g = (1 - eta/2) u^3,   u = 1/(1-eta)
//   G = kd1 I1 + kd2 C I2,   C = 1/D,  D = 1 + m A - (m-1) B,  A = (8 eta - 2 eta^2) u^4,  B = poly u^2 w^2,  w = 1/(2-eta)
// Their first and second eta-derivatives in closed form (checked symbolically) cost about a third of the generic
// value/d1/d2 arithmetic: HS' = (4-2eta)u^3, HS'' = (10-4eta)u^4, (ln g)' = 3u - w, (ln g)'' = 3u^2 - w^2,
// A' = (8+20eta-4eta^2)u^5, A'' = (60+72eta-12eta^2)u^6, and with q = u^2 w^2, s = u + w:
// B' = q (poly' + 2 poly s), B'' = 2 q s (poly' + 2 poly s) + q (poly'' + 2 poly' s + 2 poly (u^2 + w^2)).
// D2 = false everywhere below: value and first derivative only (two-term recurrences, no a''), the form of the lean
// coupled iterations; mirrors the D1s specialisation of pure_a (pure_model.hpp).
template <int N, bool D2>
PCS_DEV void horner3f(const float* coef, float x, float& p, float& d1, float& d2) {  // p, p', p''
    p = coef[N - 1];
    d1 = 0.0f;
    float h = 0.0f;
#pragma unroll
    for (int i = N - 2; i >= 0; i--) {
        if (D2) h = fmaf(h, x, d1);
        d1 = fmaf(d1, x, p);
        p = fmaf(p, x, coef[i]);
    }
    d2 = 2.0f * h;
}
template <bool D2>
PCS_DEV F2 core_closed_f32(const PureCoefF& c, float rho) {
    const float eta = rho * c.ceta;
    const float u = __builtin_amdgcn_rcpf(1.0f - eta), w = __builtin_amdgcn_rcpf(2.0f - eta);
    const float u2 = u * u, u3 = u2 * u, u4 = u2 * u2, w2 = w * w;
    const float HS = eta * (4.0f - 3.0f * eta) * u2, HS1 = (4.0f - 2.0f * eta) * u3;
    const float LG = f_log((1.0f - 0.5f * eta) * u3), LG1 = 3.0f * u - w;
    const float F = c.m * HS - c.mm1 * LG, F1_ = c.m * HS1 - c.mm1 * LG1;
    float I1, I1a, I1b, I2, I2a, I2b;
    horner3f<7, D2>(c.ai, eta, I1, I1a, I1b);
    horner3f<7, D2>(c.bi, eta, I2, I2a, I2b);
    const float A = eta * (8.0f - 2.0f * eta) * u4, A1 = (8.0f + eta * (20.0f - 4.0f * eta)) * (u4 * u);
    const float poly = eta * (20.0f + eta * (-27.0f + eta * (12.0f - 2.0f * eta)));
    const float poly1 = 20.0f + eta * (-54.0f + eta * (36.0f - 8.0f * eta));
    const float q = u2 * w2, s = u + w;
    const float t = poly1 + 2.0f * poly * s;
    const float B = poly * q, B1 = q * t;
    const float D = 1.0f + c.m * A - c.mm1 * B, D1 = c.m * A1 - c.mm1 * B1;
    const float C = __builtin_amdgcn_rcpf(D), Csq = C * C;
    const float C1 = -D1 * Csq;
    const float G = c.kd1 * I1 + c.kd2 * (C * I2);
    const float G1 = c.kd1 * I1a + c.kd2 * (C1 * I2 + C * I2a);
    const float ce = c.ceta, rc = rho * ce;  // eta-derivatives -> rho-derivatives
    F2 a;
    a.v = rho * (F + rho * G);
    a.d1 = F + rc * F1_ + rho * (2.0f * G + rc * G1);
    a.d2 = 0.0f;
    if (D2) {
        const float HS2 = (10.0f - 4.0f * eta) * u4, LG2 = 3.0f * u2 - w2;
        const float F2_ = c.m * HS2 - c.mm1 * LG2;
        const float A2 = (60.0f + eta * (72.0f - 12.0f * eta)) * (u4 * u2);
        const float poly2 = -54.0f + eta * (72.0f - 24.0f * eta);
        const float B2 = q * (2.0f * s * t + poly2 + 2.0f * poly1 * s + 2.0f * poly * (u2 + w2));
        const float D2_ = c.m * A2 - c.mm1 * B2;
        const float C2 = (2.0f * D1 * D1 * C - D2_) * Csq;
        const float G2 = c.kd1 * I1b + c.kd2 * (C2 * I2 + 2.0f * C1 * I2a + C * I2b);
        a.d2 = ce * (2.0f * F1_ + rc * F2_) + 2.0f * G + rc * (4.0f * G1 + rc * G2);
    }
    return a;
}

// Site fractions XA, XB of a pure component at S = rho Delta from the cancellation-free closed forms of pure_model.hpp.
PCS_DEV void assoc_sites_f32(const PureCoefF& c, float S, float& xa, float& xb) {
    const float sa = c.na * S, sb = c.nb * S;  // rho_a Delta, rho_b Delta
    const float t = sb - sa;
    const float aux = 1.0f - t;
    const float sq = __builtin_amdgcn_sqrtf(fmaf(aux, aux, 4.0f * sb));
    if (t > 0.5f) {
        xa = 2.0f * __builtin_amdgcn_rcpf(sq + 1.0f + t);
        xb = (sq - 1.0f + t) * __builtin_amdgcn_rcpf(2.0f * sb);
    } else if (t < -0.5f) {
        xa = (sq - 1.0f - t) * __builtin_amdgcn_rcpf(2.0f * sa);
        xb = 2.0f * __builtin_amdgcn_rcpf(sq + 1.0f - t);
    } else {
        xa = 2.0f * __builtin_amdgcn_rcpf(sq + 1.0f + t);
        xb = 2.0f * __builtin_amdgcn_rcpf(sq + 1.0f - t);
    }
}

// Association term of a pure component in closed form (value, first and second density derivative).
//   a_assoc = rho q(S),  q = na (ln XA - XA/2 + 1/2) + nb (ln XB - XB/2 + 1/2),  S = rho Delta(eta) = rho da h(eta),
//   h = u + 1.5 eta u^2 + 0.5 eta^2 u^3,  u = 1/(1-eta)                                  (pcsaft_pure.py:163-176)
// XA = 1/(1 + nb S XB), XB = 1/(1 + na S XA) depend on rho through S only.  The association energy is stationary in the
// site fractions at the mass-action solution (Michelsen's Q function), so
//   dq/dS = -na nb XA XB,   d2q/dS2 = -na nb (XA' XB + XA XB'),
//   XA' = alpha (beta S XA - XB) / (1 - alpha beta S^2),  XB' = beta (alpha S XB - XA) / (1 - alpha beta S^2),
//   alpha = nb XA^2, beta = na XB^2,
// and a' = q + rho q_S S',  a'' = 2 q_S S' + rho (q_SS S'^2 + q_S S''),  S' = da (h + eta h'),  S'' = da ceta (2 h' + eta h''),
//   h' = 2.5 u^2 + 4 eta u^3 + 1.5 eta^2 u^4,   h'' = 9 u^3 + 15 eta u^4 + 6 eta^2 u^5.
// About a third of the generic value/d1/d2 arithmetic of the term (checked against it: tests/test_pure_gpu.py goldens and
// the 1e6-row parity runs).  XA, XB themselves from the cancellation-free closed forms of pure_model.hpp.
template <bool D2>
PCS_DEV F2 assoc_closed_f32(const PureCoefF& c, float rho) {
    const float eta = rho * c.ceta;
    const float u = __builtin_amdgcn_rcpf(1.0f - eta);
    const float u2 = u * u, eu = eta * u;
    const float h = u * (1.0f + eu * (1.5f + 0.5f * eu));
    const float h1 = u2 * (2.5f + eu * (4.0f + 1.5f * eu));
    const float S = rho * c.da * h;
    const float S1 = c.da * (h + eta * h1);
    float xa, xb;
    assoc_sites_f32(c, S, xa, xb);
    const float q = c.na * (f_log(xa) - 0.5f * xa + 0.5f) + c.nb * (f_log(xb) - 0.5f * xb + 0.5f);
    const float nn = c.na * c.nb;
    const float q1 = -nn * xa * xb;
    F2 r;
    r.v = rho * q;
    r.d1 = q + rho * q1 * S1;
    r.d2 = 0.0f;
    if (D2) {
        const float h2 = u2 * u * (9.0f + eu * (15.0f + 6.0f * eu));
        const float S2 = c.da * c.ceta * (2.0f * h1 + eta * h2);
        const float al = c.nb * xa * xa, be = c.na * xb * xb;
        const float rden = __builtin_amdgcn_rcpf(1.0f - al * be * S * S);
        const float xa1 = al * (be * S * xa - xb) * rden, xb1 = be * (al * S * xb - xa) * rden;
        const float q2 = -nn * (xa1 * xb + xa * xb1);
        r.d2 = 2.0f * q1 * S1 + rho * (q2 * S1 * S1 + q1 * S2);
    }
    return r;
}

// same model as pure_a() (pure_model.hpp), fp32
PCS_DEV EvalF pure_eval_f32(const PureCoefF& c, float rho) {
    F2 a = core_closed_f32<true>(c, rho);
    if (c.polar || c.assoc) {
        F2 r = f2(rho, 1.0f, 0.0f);
        F2 eta = r * c.ceta;
        if (c.polar) {
            F2 rho2 = r * r;
            F2 J1 = hornerf<5>(c.j1, eta);
            F2 J2 = hornerf<4>(c.j2, eta);
            a = a + (rho2 * c.qm) * ((J1 * J1) * recipf(J1 - r * J2));
        }
        if (c.assoc) {
            a = a + assoc_closed_f32<true>(c, rho);
        }
    }
    EvalF ec;
    ec.a = a.v;
    ec.p = rho - a.v + rho * a.d1;
    ec.dp = 1.0f + rho * a.d2;
    ec.mu = a.d1;
    return ec;
}

// The same without a'': a, p and mu = a' (no dp/drho).  About two thirds of the arithmetic of pure_eval_f32.
struct EvalF1 { float a, p, mu; };
PCS_DEV EvalF1 pure_eval1_f32(const PureCoefF& c, float rho) {
    const F2 core = core_closed_f32<false>(c, rho);
    float a = core.v, a1 = core.d1;
    if (c.polar || c.assoc) {
        if (c.polar) {
            const F1 r = f1(rho, 1.0f);
            const F1 eta = r * c.ceta;
            const F1 J1 = hornerf<5>(c.j1, eta);
            const F1 J2 = hornerf<4>(c.j2, eta);
            const F1 d = ((r * r) * c.qm) * ((J1 * J1) * recipf(J1 - r * J2));
            a += d.v;
            a1 += d.d1;
        }
        if (c.assoc) {
            const F2 as = assoc_closed_f32<false>(c, rho);
            a += as.v;
            a1 += as.d1;
        }
    }
    EvalF1 e;
    e.a = a;
    e.p = rho - a + rho * a1;
    e.mu = a1;
    return e;
}

// ------------------------------------------------------------------------------------------------------------------------
// The evaluation at the start density of the liquid root.  Every lane starts at rho0 = PCS_F32_START_ETA / ceta, i.e. at
// the same packing fraction eta0, where everything in the closed forms above that depends on eta alone is a number: u, w and
// their powers, HS, ln g, A, B with their derivatives (two reciprocals and the logarithm), and the polynomials I1, I2, whose
// coefficients are ai[i] = A0[i] + m1 (A1[i] + m2 A2[i]), reduce to three eta-moments of the universal tables each.  The
// derivatives are taken in t = rho / rho0 at t = 1 (x_t = rho x', x_tt = rho^2 x''): eta_t = eta0, so the chain-rule factors
// are numbers as well, and p = rho0 - a + a_t, a' = a_t / rho0, dp/drho = 1 + a_tt / rho0.  All constants are derived here at
// compile time, in double, from PCS_F32_START_ETA and pcsaft_consts.hpp.
constexpr float PCS_F32_START_ETA = 0.5f;

struct StartMom { double v, t, tt; };  // x, eta x', eta^2 x'' at eta0
struct StartPow { float v[7], t[7], tt[7]; };  // eta0^i, i eta0^i, i (i-1) eta0^i
struct StartConst {
    double u;                   // 1 / (1 - eta0)
    StartMom HS, LG, A, B, H;   // H: S = rho Delta = rho0 da t h(eta0 t) -> S, S_t, S_tt in units of rho0 da
    StartMom SA[3], SB[3];      // moments of A0, A1, A2 / B0, B1, B2
    StartPow pw;
};
constexpr double start_atanh2(double z) {  // 2 atanh(z), |z| <= 1/3
    double sum = 0.0, zp = z;
    for (int k = 1; k < 80; k += 2) { sum += zp / k; zp *= z * z; }
    return 2.0 * sum;
}
constexpr double start_log(double x) {  // ln x, x > 0
    int k = 0;
    while (x > 1.5) { x *= 0.5; k++; }
    while (x < 0.75) { x *= 2.0; k--; }
    return k * start_atanh2(1.0 / 3.0) + start_atanh2((x - 1.0) / (x + 1.0));
}
template <int N>
constexpr StartMom start_moments(const double (&c)[N], double e) {
    StartMom r = {0.0, 0.0, 0.0};
    double pw = 1.0;
    for (int i = 0; i < N; i++) { r.v += c[i] * pw; r.t += i * c[i] * pw; r.tt += i * (i - 1) * c[i] * pw; pw *= e; }
    return r;
}
template <int N>
constexpr StartMom start_horner(const double (&c)[N], double e) {  // the recurrences of horner3f
    double p = c[N - 1], d1 = 0.0, h = 0.0;
    for (int i = N - 2; i >= 0; i--) { h = h * e + d1; d1 = d1 * e + p; p = p * e + c[i]; }
    return StartMom{p, e * d1, e * e * 2.0 * h};
}
constexpr bool start_close(double a, double b) { return (a - b) * (a - b) <= 1e-24 * (1.0 + a * a); }
constexpr bool start_close(const StartMom& a, const StartMom& b) { return start_close(a.v, b.v) && start_close(a.t, b.t) && start_close(a.tt, b.tt); }
constexpr StartConst start_const(double e) {
    StartConst k = {};
    const double u = 1.0 / (1.0 - e), w = 1.0 / (2.0 - e);
    const double u2 = u * u, u3 = u2 * u, u4 = u2 * u2, w2 = w * w;
    k.u = u;
    k.HS = StartMom{e * (4.0 - 3.0 * e) * u2, e * (4.0 - 2.0 * e) * u3, e * e * (10.0 - 4.0 * e) * u4};
    k.LG = StartMom{start_log((1.0 - 0.5 * e) * u3), e * (3.0 * u - w), e * e * (3.0 * u2 - w2)};
    k.A = StartMom{e * (8.0 - 2.0 * e) * u4, e * (8.0 + e * (20.0 - 4.0 * e)) * (u4 * u), e * e * (60.0 + e * (72.0 - 12.0 * e)) * (u4 * u2)};
    const double poly = e * (20.0 + e * (-27.0 + e * (12.0 - 2.0 * e)));
    const double poly1 = 20.0 + e * (-54.0 + e * (36.0 - 8.0 * e)), poly2 = -54.0 + e * (72.0 - 24.0 * e);
    const double q = u2 * w2, s = u + w, t = poly1 + 2.0 * poly * s;
    k.B = StartMom{poly * q, e * (q * t), e * e * (q * (2.0 * s * t + poly2 + 2.0 * poly1 * s + 2.0 * poly * (u2 + w2)))};
    const double eu = e * u;
    const double h = u * (1.0 + eu * (1.5 + 0.5 * eu)), h1 = u2 * (2.5 + eu * (4.0 + 1.5 * eu)), h2 = u3 * (9.0 + eu * (15.0 + 6.0 * eu));
    k.H = StartMom{h, h + e * h1, 2.0 * e * h1 + e * e * h2};
    k.SA[0] = start_moments(A0, e); k.SA[1] = start_moments(A1, e); k.SA[2] = start_moments(A2, e);
    k.SB[0] = start_moments(B0, e); k.SB[1] = start_moments(B1, e); k.SB[2] = start_moments(B2, e);
    double pw = 1.0;
    for (int i = 0; i < 7; i++) { k.pw.v[i] = (float)pw; k.pw.t[i] = (float)(i * pw); k.pw.tt[i] = (float)(i * (i - 1) * pw); pw *= e; }
    return k;
}
constexpr StartConst START = start_const((double)PCS_F32_START_ETA);
static_assert(PCS_F32_START_ETA > 0.0f && PCS_F32_START_ETA < 1.0f, "start packing fraction");
static_assert(start_close(START.SA[0], start_horner(A0, (double)PCS_F32_START_ETA)) && start_close(START.SA[1], start_horner(A1, (double)PCS_F32_START_ETA)) &&
              start_close(START.SA[2], start_horner(A2, (double)PCS_F32_START_ETA)), "eta-moments of A0..A2 against their Horner evaluation");
static_assert(start_close(START.SB[0], start_horner(B0, (double)PCS_F32_START_ETA)) && start_close(START.SB[1], start_horner(B1, (double)PCS_F32_START_ETA)) &&
              start_close(START.SB[2], start_horner(B2, (double)PCS_F32_START_ETA)), "eta-moments of B0..B2 against their Horner evaluation");
static_assert(start_close(start_log(6.0), 2.0 * start_log(2.0) + start_log(1.5)) && start_close(start_log(0.001) + start_log(1000.0), 0.0) &&
              start_close(start_log(2.718281828459045), 1.0), "compile-time logarithm");

PCS_DEV float start_rho_f32(const PureCoefF& c) { return PCS_F32_START_ETA / c.ceta; }

// (a, p, dp, mu) of pure_eval_f32(c, start_rho_f32(c)); what remains per row is linear in m, m-1, m1, m1 m2, the reciprocal of
// D, the dot products of the row's dipole coefficients with the powers of eta0, and the site fractions.
PCS_DEV EvalF pure_eval_start_f32(const PureCoefF& c) {
    constexpr StartConst K = START;
    const float rho = start_rho_f32(c);
    const float F = c.m * (float)K.HS.v - c.mm1 * (float)K.LG.v;
    const float Ft = c.m * (float)K.HS.t - c.mm1 * (float)K.LG.t;
    const float Ftt = c.m * (float)K.HS.tt - c.mm1 * (float)K.LG.tt;
    const float m1 = c.m1, m2 = c.m2;
    const float I1 = fmaf(m1, fmaf(m2, (float)K.SA[2].v, (float)K.SA[1].v), (float)K.SA[0].v);
    const float I1t = fmaf(m1, fmaf(m2, (float)K.SA[2].t, (float)K.SA[1].t), (float)K.SA[0].t);
    const float I1tt = fmaf(m1, fmaf(m2, (float)K.SA[2].tt, (float)K.SA[1].tt), (float)K.SA[0].tt);
    const float I2 = fmaf(m1, fmaf(m2, (float)K.SB[2].v, (float)K.SB[1].v), (float)K.SB[0].v);
    const float I2t = fmaf(m1, fmaf(m2, (float)K.SB[2].t, (float)K.SB[1].t), (float)K.SB[0].t);
    const float I2tt = fmaf(m1, fmaf(m2, (float)K.SB[2].tt, (float)K.SB[1].tt), (float)K.SB[0].tt);
    const float D = 1.0f + c.m * (float)K.A.v - c.mm1 * (float)K.B.v;
    const float Dt = c.m * (float)K.A.t - c.mm1 * (float)K.B.t;
    const float Dtt = c.m * (float)K.A.tt - c.mm1 * (float)K.B.tt;
    const float C = __builtin_amdgcn_rcpf(D), Csq = C * C;
    const float Ct = -Dt * Csq;
    const float Ctt = (2.0f * Dt * Dt * C - Dtt) * Csq;
    const float G = c.kd1 * I1 + c.kd2 * (C * I2);
    const float Gt = c.kd1 * I1t + c.kd2 * (Ct * I2 + C * I2t);
    const float Gtt = c.kd1 * I1tt + c.kd2 * (Ctt * I2 + 2.0f * Ct * I2t + C * I2tt);
    float a = rho * (F + rho * G);
    float at = rho * (F + Ft + rho * (2.0f * G + Gt));
    float att = rho * (2.0f * Ft + Ftt + rho * (2.0f * G + 4.0f * Gt + Gtt));
    if (c.polar || c.assoc) {
        if (c.polar) {
            // a = rho^2 qm J1^2 / (J1 - rho J2) = (rho0^2 qm) t^2 Q(t),  Q = J1^2 / (J1 - t N),  N = rho0 J2
            float j1v = c.j1[0], j1t = 0.0f, j1tt = 0.0f, j2v = c.j2[0], j2t = 0.0f, j2tt = 0.0f;
#pragma unroll
            for (int i = 1; i < 5; i++) {
                j1v = fmaf(c.j1[i], K.pw.v[i], j1v);
                j1t = fmaf(c.j1[i], K.pw.t[i], j1t);
                if (i > 1) j1tt = fmaf(c.j1[i], K.pw.tt[i], j1tt);
            }
#pragma unroll
            for (int i = 1; i < 4; i++) {
                j2v = fmaf(c.j2[i], K.pw.v[i], j2v);
                j2t = fmaf(c.j2[i], K.pw.t[i], j2t);
                if (i > 1) j2tt = fmaf(c.j2[i], K.pw.tt[i], j2tt);
            }
            const F2 J1 = f2(j1v, j1t, j1tt);
            const F2 N = f2(j2v, j2t, j2tt) * rho;
            const F2 Q = (J1 * J1) * recipf(J1 - f2(N.v, N.d1 + N.v, N.d2 + 2.0f * N.d1));
            const float k = (rho * rho) * c.qm;
            a = fmaf(k, Q.v, a);
            at = fmaf(k, Q.d1 + 2.0f * Q.v, at);
            att = fmaf(k, Q.d2 + 4.0f * Q.d1 + 2.0f * Q.v, att);
        }
        if (c.assoc) {
            // assoc_closed_f32 with S, S_t, S_tt = (rho0 da) (h, h + eta0 h', 2 eta0 h' + eta0^2 h'')
            const float rd = rho * c.da;
            const float S = rd * (float)K.H.v, St = rd * (float)K.H.t, Stt = rd * (float)K.H.tt;
            float xa, xb;
            assoc_sites_f32(c, S, xa, xb);
            const float q = c.na * (f_log(xa) - 0.5f * xa + 0.5f) + c.nb * (f_log(xb) - 0.5f * xb + 0.5f);
            const float nn = c.na * c.nb;
            const float q1 = -nn * xa * xb;
            const float al = c.nb * xa * xa, be = c.na * xb * xb;
            const float rden = __builtin_amdgcn_rcpf(1.0f - al * be * S * S);
            const float xa1 = al * (be * S * xa - xb) * rden, xb1 = be * (al * S * xb - xa) * rden;
            const float q2 = -nn * (xa1 * xb + xa * xb1);
            a = fmaf(rho, q, a);
            at = fmaf(rho, q + q1 * St, at);
            att = fmaf(rho, q1 * (2.0f * St + Stt) + q2 * St * St, att);
        }
    }
    const float ir = c.ceta * (1.0f / PCS_F32_START_ETA);  // 1 / rho0
    EvalF e;
    e.a = a;
    e.p = rho - a + at;
    e.dp = fmaf(att, ir, 1.0f);
    e.mu = at * ir;
    return e;
}

PCS_DEV bool finitef(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// What the pre-solve did on a row, for the row order (pcs_pure_row_order sorts on it) and its probe; the solving kernels
// pass no PreSignature and none of this is computed there.  Margins are quotients value / threshold of the pre-solve's own
// stop decisions: <= 1 means the decision fell on the cheap side.
constexpr float PRE_MARGIN_OPEN = 1e30f;  // the decision was never reached on its cheap side (restart, failure)
enum : int { PRE_SIG_REEVAL = 1, PRE_SIG_FULL_V = 2 };
struct PreSignature {
    int n_liq, n_cpl, code;  // liquid-root evaluations (0..12), coupled iterations (0..8), failure code (0: none)
    int flags;               // PRE_SIG_REEVAL / PRE_SIG_FULL_V: a full liquid / vapour evaluation in a coupled iteration >= 2
    float m_liq;             // liquid root, second evaluation: |scaled Newton step| / (tolerance rho); 0 when the first one ended it
    float m_l, m_v;          // second coupled iteration: max(pl / PCS_F32_PREDICT_TOL_L, sl / 1e-2), max(pv / PCS_F32_PREDICT_TOL_V, sv / 1e-2); 0: not run
};

struct LiquidRootF {
    float rl;
    bool ok, done, dense;
    int first;  // iteration at which the current start density is evaluated
    float m2;   // signature only: step of the second evaluation over its tolerance (0: done at the first, huge: no Newton step there)
};
// One iteration of liquid_root_f32 from the evaluation `e` at s.rl.  AT_START: s.rl is the start density (iteration 0).
template <bool AT_START, bool SIG = false>
PCS_DEV void liquid_root_step(const PureCoefF& f, float p_spec, float tol, float tol_dense, int it, const EvalF& e, LiquidRootF& s) {
    const float res = e.p - p_spec;
    // rung of the ladder eta = 0.58, 0.66, 0.74 above this start (a start within 0.005 below a rung takes the one after it, so
    // every restart moves up; PCS_F32_DENSE_LEVELS: none left)
    const float eta = AT_START ? PCS_F32_START_ETA : s.rl * f.ceta;
    const int rung = AT_START ? 0 : eta < 0.575f ? 0 : eta < 0.655f ? 1 : eta < 0.735f ? 2 : PCS_F32_DENSE_LEVELS;
    if (it == s.first && rung < PCS_F32_DENSE_LEVELS && finitef(e.p) && !(res > 0.0f)) {
        // still on the dilute side of the root: the next start lies on its dense side
        s.dense = true;
        s.first = it + 1;
        float rn = (0.58f + 0.08f * (float)rung) / f.ceta;
        if (AT_START && e.dp > 0.0f) {
            // on the liquid branch below the root, p convex from here on (hard-sphere pole): the plain Newton point lies above
            // the root and costs no evaluation; the ladder stays behind it (an evaluation there that is still not above the
            // root -- second loop of strongly polar sets -- goes on to the rung above it)
            const float r1 = s.rl - res * __builtin_amdgcn_rcpf(e.dp);
            const float eta1 = r1 * f.ceta;
            if (finitef(r1) && eta1 > PCS_F32_START_ETA && eta1 <= 0.74f) rn = r1;
        }
        s.rl = rn;
    } else if (!finitef(e.p) || !(e.dp > 0.0f) || (it == s.first && !(res > 0.0f))) {
        s.ok = false;
        s.done = true;
    } else {
        const float u = AT_START ? (float)START.u : __builtin_amdgcn_rcpf(1.0f - s.rl * f.ceta);
        float den = s.dense ? e.dp : e.dp - 4.0f * res * f.ceta * u;
        float step = res * __builtin_amdgcn_rcpf(den);
        if (!(den > 0.0f)) step = 2.0f * s.rl;  // -> rn < 0 -> this lane takes the fp64 initialiser
        float rn = s.rl - step;
        if (!(rn > 0.0f)) { s.ok = false; s.done = true; }
        else {
            s.done = fabsf(step) <= (s.dense ? tol_dense : tol) * s.rl;
            if constexpr (SIG) {
                if (AT_START) s.m2 = s.done ? 0.0f : PRE_MARGIN_OPEN;
                else if (it == 1) s.m2 = fabsf(step) * __builtin_amdgcn_rcpf((s.dense ? tol_dense : tol) * s.rl);
            }
            s.rl = rn;
        }
    }
}
// fp32 liquid root of p(rho) = p_spec from eta = 0.5.  Newton on (p - p_spec)(1-eta)^4 = 0 (same root):
// the hard-sphere pole makes p(rho) very steep on the dense side, the scaled function is close to
// linear -> 2-3 evaluations instead of 4-6 to a 10 % step.  Strongly attractive rows (large dipole /
// association at low T) have their liquid above eta = 0.5: they restart on its dense side, at the plain Newton point
// from eta = 0.5 (p is convex there, so the point lies above the root; no evaluation spent on finding one) or, where
// that point is unusable or still below the root, on the ladder eta = 0.58, 0.66, 0.74, and go on with plain Newton
// (monotone from there) and the tighter `tol_dense`.
// Wave-uniform loop; returns false when the lane must use the fp64 initialiser.  Iteration 0 is peeled: every lane is at
// eta0 there and takes pure_eval_start_f32.
template <bool SIG = false>
PCS_DEV bool liquid_root_f32(const PureCoefF& f, float p_spec, float tol, float tol_dense, int cap, float& rl,
                             int& n_eval, float* m2 = nullptr) {
    LiquidRootF s;
    if constexpr (SIG) s.m2 = PRE_MARGIN_OPEN;
    s.ok = finitef(f.da) && finitef(f.kd2) && finitef(f.ceta) && f.ceta > 0.0f && finitef(p_spec);
    s.rl = start_rho_f32(f);
    s.done = !s.ok;
    s.dense = false;
    s.first = 0;
    // iteration 0: every lane is at eta0 -> the fixed-eta evaluation (wave-uniform, no second body per lane).  The
    // dense-side restarts share their iterations with other lanes' Newton evaluations and stay generic.
    if (cap > 0) {
        if (!s.done) {
            liquid_root_step<true, SIG>(f, p_spec, tol, tol_dense, 0, pure_eval_start_f32(f), s);
            n_eval++;
        }
        if (__ballot(!s.done) != 0ull) {
#pragma unroll 1
            for (int it = 1; it < cap; it++) {
                if (!s.done) {
                    liquid_root_step<false, SIG>(f, p_spec, tol, tol_dense, it, pure_eval_f32(f, s.rl), s);
                    n_eval++;
                }
                if (__ballot(!s.done) == 0ull) break;
            }
        }
    }
    rl = s.rl;
    if constexpr (SIG) *m2 = s.m2;
    return s.ok && s.done;
}

// fp32 pass, in two parts (vle_presolve_f32 below runs one after the other; nothing resumes a lane in between):
//   presolve_begin:   zero-pressure liquid root, liquid state at it, virial-corrected ideal-gas vapour estimate
//   presolve_coupled: coupled Newton towards the equal-area pressure from iteration s.it up to (excluding) it_end, or
//                     until every lane of the wave is done
// vle_presolve_f32 = begin + coupled(8).  s.ok: every step behaved (otherwise the lane uses the fp64 initialiser);
// s.done && s.ok: converged to the fp32 noise floor (typically 1e-6 relative).  Not converged within the cap is fine: the
// fp64 iteration continues from there.  l.dp / dpv: dp/drho of the two phases from the last evaluations (one small step
// before the returned densities): the second derivative the fp64 finish uses for its Newton steps.
struct PreState {
    float rl, rv;
    EvalF l;              // liquid state at rl (re-evaluated or carried by the Taylor expansion)
    float dpv;            // dp/drho of the vapour at its last evaluation
    float sl_prev, sv_prev;
    float pv, dv_taken;   // vapour pressure at its last evaluation and the step taken from there (carry_slope)
    float ev;             // estimated relative error of the carried slope dpv (0 after a full evaluation)
    float sec_prev, d_prev;  // the last pressure quotient and its step (d_prev = 0: none since the last full evaluation)
    bool lean_v;          // the lane's next vapour evaluation may be the one without the second derivative
    int it, n_liq, code;  // coupled iterations done; diagnostics
    bool ok, done;
    float m_liq, m_l, m_v;  // signature only (PreSignature)
    int flags;
};

template <bool SIG = false>
PCS_DEV void presolve_begin(const PureCoefF& f, PreState& s) {
    s.n_liq = 0; s.it = 0; s.code = 0;
    if constexpr (SIG) { s.m_liq = PRE_MARGIN_OPEN; s.m_l = 0.0f; s.m_v = 0.0f; s.flags = 0; }
    s.dpv = 1.0f; s.sl_prev = 1.0f; s.sv_prev = 1.0f;
    s.pv = 0.0f; s.dv_taken = 0.0f; s.ev = 0.0f; s.sec_prev = 0.0f; s.d_prev = 0.0f; s.lean_v = false;
    // zero-pressure liquid, handed over to the coupled iteration at a loose step
    bool ok = liquid_root_f32<SIG>(f, 0.0f, PCS_F32_LIQ_TOL, 1e-2f, 12, s.rl, s.n_liq, &s.m_liq);
    const float rl = s.rl;
    s.l = pure_eval_f32(f, rl);
    float rv = rl * f_exp(s.l.mu);
    {
        // second-virial correction of the ideal-gas estimate: ln rho + 2 B rho = ln rho_L + mu_L^res with
        // B = lim a/rho^2 from the coefficients (no model evaluation); three scalar Newton steps
        float B = (4.0f * f.m - 2.5f * f.mm1) * f.ceta + f.kd1 * f.ai[0] + f.kd2 * f.bi[0];
        if (f.polar) B += f.qm * f.j1[0];
        if (f.assoc) B -= f.na * f.nb * f.da;
        const float Lg = f_log(rv);
        float r = rv;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            float den = fmaxf(1.0f + 2.0f * B * r, 0.3f);
            float fr = f_log(r) + 2.0f * B * r - Lg;
            r = r * fmaxf(1.0f - fr * __builtin_amdgcn_rcpf(den), 0.2f);
        }
        if (finitef(r) && r > 0.0f) rv = r;
    }
    s.code = !ok ? 1 : !finitef(rv) ? 6 : !(s.l.dp > 0.0f) ? 7 : !(rv < 0.5f * rl) ? 8 : !(rv > 1e-30f) ? 9 : 0;
    ok = ok && finitef(rv) && (s.l.dp > 0.0f) && (rv < 0.5f * rl) && (rv > 1e-30f);
    s.rv = rv;
    s.ok = ok;
    s.done = !ok;
}

// Update of the carried vapour slope dp (at the last evaluation, pressure p0) from the pressure p1 one step `drho` further.
// First update after a full evaluation (d_prev == 0): the trapezoid rule 2 (p1 - p0)/drho - dp, dp/drho at the new point up
// to p''' drho^2 / 12.  Later updates: the derivative at the new point of the parabola through the last three evaluations,
// from the two quotients sec_prev (over d_prev) and sec (over drho): sec + (sec - sec_prev) drho / (d_prev + drho), error
// ~ p''' d_prev drho / 6 -- it forgets the error of the older slope as the steps shrink; taken only when the step has at
// least halved (two steps of opposite sign and like size would divide by their small sum).  `s` = |drho|/rho of the step,
// `mu` = a' at the new point (noise model: PCS_F32_SECANT_MIN); a step below the noise threshold keeps the slope.
// Returns false when the result is unusable (not finite or not positive: the lane then takes the full evaluation at the
// same density).  `err`: estimated relative error of the slope, a quarter of the squared relative change after a
// trapezoid update (three times the rule's own term), the geometric mean of that and the previous estimate afterwards.
PCS_DEV bool carry_slope(float p0, float p1, float drho, float s, float mu, float& dp, float& err, float& sec_prev, float& d_prev) {
    if (!(s * dp >= PCS_F32_SECANT_MIN * (1.0f + fabsf(mu)))) {
        d_prev = 0.0f;
        return true;
    }
    const float sec = (p1 - p0) * __builtin_amdgcn_rcpf(drho);
    const bool three = d_prev != 0.0f && fabsf(drho) <= 0.5f * fabsf(d_prev);
    const float cand = three ? fmaf(sec - sec_prev, drho * __builtin_amdgcn_rcpf(d_prev + drho), sec) : fmaf(2.0f, sec, -dp);
    if (!finitef(cand) || !(cand > 0.0f)) return false;
    const float rel = fabsf(cand * __builtin_amdgcn_rcpf(dp) - 1.0f);
    err = three ? 0.5f * rel * __builtin_amdgcn_sqrtf(err) : 0.25f * rel * rel;
    dp = cand;
    sec_prev = sec;
    d_prev = drho;
    return true;
}

template <bool SIG = false>
PCS_DEV void presolve_coupled(const PureCoefF& f, PreState& s, int it_end) {
    float rl = s.rl, rv = s.rv;
    EvalF l = s.l;
    bool ok = s.ok, done = s.done;
    float dpv_last = s.dpv, dl_taken = 0.0f;
    float sl_prev = s.sl_prev, sv_prev = s.sv_prev;
    float pv_last = s.pv, dv_taken = s.dv_taken, ev = s.ev, sec_prev = s.sec_prev, d_prev = s.d_prev;
    bool lean_v = s.lean_v;
    int n_cpl = s.it;
    float m_l = 0.0f, m_v = 0.0f;  // signature only
    int flags = 0;
    if constexpr (SIG) { m_l = s.m_l; m_v = s.m_v; flags = s.flags; }
    // `it` below only bounds the loop, the lane's own count n_cpl decides what the first-iteration rule of the stop
    // criterion sees
    for (int it = 0; it < it_end; it++) {
        const bool act = !done && n_cpl < it_end;
        // Vapour evaluation.  A lane's first one computes a, a', a'' (pure_eval_f32).  From its second iteration on
        // a'' -- used for dp/drho, the slope of the Newton step, only -- is not computed: the lane evaluates a and a'
        // (pure_eval1_f32) and carries the slope (carry_slope), unless its last step was taken in ln(rho) or was larger
        // than PCS_F32_LEAN_MAX, or the carried slope turns out unusable.  The choice depends on the lane's own state
        // only; a form is executed when some lane of the wave takes it.
        EvalF v;
        v.a = 0.0f; v.p = 0.0f; v.mu = 0.0f;
        bool full = act && !lean_v;
        const bool lean = act && lean_v;
        if (__ballot(lean) != 0ull) {
            if (lean) {
                const EvalF1 e = pure_eval1_f32(f, rv);
                v.a = e.a; v.p = e.p; v.mu = e.mu;
                full = !carry_slope(pv_last, e.p, dv_taken, sv_prev, e.mu, dpv_last, ev, sec_prev, d_prev);
            }
        }
        if (__ballot(full) != 0ull) {
            if (full) {
                v = pure_eval_f32(f, rv);
                if constexpr (SIG) { if (n_cpl >= 1) flags |= PRE_SIG_FULL_V; }
                dpv_last = v.dp;
                ev = 0.0f;
                d_prev = 0.0f;
            }
        }
        if (act) {
            v.dp = dpv_last;
            pv_last = v.p;
            float iv = __builtin_amdgcn_rcpf(rv), il = __builtin_amdgcn_rcpf(rl);
            float ps = -(v.a * iv - l.a * il + f_log(rv * il)) * __builtin_amdgcn_rcpf(iv - il);
            float dl = -(l.p - ps) * __builtin_amdgcn_rcpf(l.dp);
            float dv = -(v.p - ps) * __builtin_amdgcn_rcpf(v.dp);
            float rln = rl + dl, rvn = rv + dv;
            // a large downward vapour step (poor first estimate at very low pressures) is taken in ln(rho) instead
            const bool log_step = rvn < 0.3f * rv;
            if (log_step) rvn = rv * f_exp(dv * iv);
            if (!finitef(rln) || !finitef(rvn) || !(v.dp > 0.0f) || !(l.dp > 0.0f) || !(rvn > 1e-30f) || !(rvn < 0.6f * rln)) {
                s.code = (!finitef(rln) || !finitef(rvn)) ? 10 : !(v.dp > 0.0f) ? 11 : !(l.dp > 0.0f) ? 12 : !(rvn > 1e-30f) ? 13 : 14;
                ok = false;
                done = true;
            } else {
                // |next step| ~ step (C step + e): C step^2 is Newton's quadratic term with C estimated from the last two
                // steps, e step the linear term that a slope with the relative error e leaves (0 after a full evaluation)
                float sl = fabsf(dl) * il, sv = fabsf(dv) * iv;
                float pl = sl * sl * fminf(sl * __builtin_amdgcn_rcpf(sl_prev * sl_prev), PCS_F32_PREDICT_CMAX);
                float pv = sv * fmaf(sv, fminf(sv * __builtin_amdgcn_rcpf(sv_prev * sv_prev), PCS_F32_PREDICT_CMAX), ev);
                done = ((sl <= 2e-6f) && (sv <= 3e-5f)) || (n_cpl > 0 && sl < 1e-2f && sv < 1e-2f && pl <= PCS_F32_PREDICT_TOL_L && pv <= PCS_F32_PREDICT_TOL_V);
                if constexpr (SIG) if (n_cpl == 1) {
                    m_l = fmaxf(pl * (1.0f / PCS_F32_PREDICT_TOL_L), sl * 1e2f);
                    m_v = fmaxf(pv * (1.0f / PCS_F32_PREDICT_TOL_V), sv * 1e2f);
                }
                sl_prev = sl; sv_prev = sv;
                dl_taken = rln - rl;
                dv_taken = rvn - rv;
                lean_v = !log_step && sv <= PCS_F32_LEAN_MAX;
                rl = rln;
                rv = rvn;
            }
            n_cpl++;
        }
        // the liquid state follows every taken step
        // the liquid barely moves after the first iteration: a lane whose liquid step was below 1e-3 carries its
        // liquid state to the new density by the Taylor expansion (a to 2nd, p to 1st order, dp kept) instead of a
        // re-evaluation; the error (~2.5 (dl/rho)^2 in the density) is below the fp32 noise the pass stops at.  The
        // choice is per lane (a row's result does not depend on its wave-mates); the evaluation is skipped when no
        // lane of the wave needs it.  The re-evaluation is always the full one: the liquid slope is
        // steep and strongly curved (rho p''/p' ~ 10-20), and a wave rarely has no lane whose liquid step needs it.
        {
            const bool moved = act && !done;
            const bool reeval = moved && !(fabsf(dl_taken) <= PCS_F32_TAYLOR_MAX * rl);
            if (moved && !reeval) {
                const float a2 = (l.dp - 1.0f) * __builtin_amdgcn_rcpf(rl - dl_taken);  // a'' at the expansion point
                l.a = fmaf(dl_taken, fmaf(0.5f * a2, dl_taken, l.mu), l.a);
                l.mu = fmaf(a2, dl_taken, l.mu);
                l.p = fmaf(l.dp, dl_taken, l.p);
            }
            if (__ballot(reeval) != 0ull) {
                if (reeval) {
                    l = pure_eval_f32(f, rl);
                    if constexpr (SIG) { if (n_cpl >= 2) flags |= PRE_SIG_REEVAL; }
                }
            }
        }
        if (__ballot(!done && n_cpl < it_end) == 0ull) break;
    }
    s.rl = rl; s.rv = rv; s.l = l; s.dpv = dpv_last; s.sl_prev = sl_prev; s.sv_prev = sv_prev;
    s.pv = pv_last; s.dv_taken = dv_taken; s.ev = ev; s.sec_prev = sec_prev; s.d_prev = d_prev; s.lean_v = lean_v;
    s.it = n_cpl; s.ok = ok; s.done = done;
    if constexpr (SIG) { s.m_l = m_l; s.m_v = m_v; s.flags = flags; }
}

template <bool SIG = false>
PCS_DEV bool vle_presolve_f32(const PureCoefF& f, double& rl_out, double& rv_out, float& dpl_out, float& dpv_out,
                              PreSignature* sig = nullptr) {
    PreState s;
    presolve_begin<SIG>(f, s);
    presolve_coupled<SIG>(f, s, 8);
    rl_out = (double)s.rl;
    rv_out = (double)s.rv;
    dpl_out = s.l.dp;
    dpv_out = s.dpv;
    if constexpr (SIG) *sig = PreSignature{s.n_liq, s.it, s.code, s.flags, s.m_liq, s.m_l, s.m_v};  // the order kernels only
    return s.ok;
}

}  // namespace pcs
