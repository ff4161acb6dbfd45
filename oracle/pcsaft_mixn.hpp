// ORACLE — TEST INFRASTRUCTURE ONLY (see dual.hpp header).
//
// n-component PC-SAFT mixtures: CPU restatement of the parts of the reference's PcSaftMix that are written
// for any number of components --
//   helmholtz_energy_density  <- feos_torch/pcsaft_mix.py:31-154   (hs :56-60, hc :63-65, dispersion :69-106 without k_ij:
//                                "kij can only be used for binary mixtures!" :75-76, dipoles :156-208, self association of
//                                ONE associating component :210-239; two associating components are binary-only :250, :336)
//   derivatives               <- :395-420  (a, p, mu_i, v_i from one hyper-dual pass over A(N, V) = V a(N/V))
// Plain loops over the components; S is double, long double or a HyperDual.  NCMAX components at most.
// The parameter type P is double (the parameters are numbers: what orc_mixn_derivatives evaluates) or S itself (the parameters
// carry tangents like T and the densities: the exact gradient, orc_mixn_derivatives_vjp_exact).  With P = double every
// operation is the one the plain restatement always did.
#pragma once
#include <type_traits>
#include "constants.hpp"
#include "dual.hpp"
#include "pcsaft_mix.hpp"  // clamp2, pair_integral, triplet_integral, site_f

namespace oracle {

constexpr int MIXN_MAX = 6;

// a parameter-typed value where the model needs an S
template <class S, class P>
S mixn_lift(const P& x) {
    if constexpr (std::is_same<S, P>::value) return x;
    else return S(x);
}

// par [nc][8] rows (m, sigma, epsilon_k, mu, kappa_ab, epsilon_k_ab, na, nb).  Returns false through `ok` if the rows ask for
// an association class the reference only implements for binary mixtures.  The class decisions (polar? associating?
// min(m, 2)) are taken on the real parts, so a tangent on a parameter never changes the formula that is differentiated.
template <class S, class P = double>
S helmholtz_energy_density_mixn(int nc, const P* par, const S& T, const S* rho, bool& ok) {
    ok = true;
    S d[MIXN_MAX];
    P m[MIXN_MAX], sigma[MIXN_MAX], eps[MIXN_MAX], mu2[MIXN_MAX];
    for (int i = 0; i < nc; i++) {
        const P* p = par + 8 * i;
        m[i] = p[0]; sigma[i] = p[1]; eps[i] = p[2];
        mu2[i] = p[3] * p[3] / (m[i] * sigma[i] * sigma[i] * sigma[i] * eps[i]) * 1e-19 * (1.0 / KB);  // :17-22
        d[i] = sigma[i] * (1.0 - 0.12 * exp(-3.0 * mixn_lift<S, P>(eps[i]) / T));                        // :33
    }
    S zeta0(0.0), zeta1(0.0), zeta2(0.0), zeta3(0.0), rho_sum(0.0);
    for (int i = 0; i < nc; i++) {
        S mr = rho[i] * m[i];
        zeta0 = zeta0 + mr; zeta1 = zeta1 + mr * d[i]; zeta2 = zeta2 + mr * d[i] * d[i]; zeta3 = zeta3 + mr * d[i] * d[i] * d[i];
        rho_sum = rho_sum + rho[i];
    }
    zeta0 = zeta0 * (PI / 6.0); zeta1 = zeta1 * (PI / 6.0); zeta2 = zeta2 * (PI / 6.0); zeta3 = zeta3 * (PI / 6.0);  // :35-38
    S zeta23 = zeta2 / zeta3;
    S zeta3_2 = zeta3 * zeta3, zeta3_3 = zeta3_2 * zeta3;
    S zeta3_m1 = 1.0 / (1.0 - zeta3);
    S zeta3_m2 = zeta3_m1 * zeta3_m1;
    S etas[7] = {S(1.0), zeta3, zeta3_2, zeta3_3, zeta3_2 * zeta3_2, zeta3_2 * zeta3_3, zeta3_3 * zeta3_3};
    // hard sphere (:56-60)
    S phi = (6.0 / PI) * (zeta1 * zeta2 * zeta3_m1 * 3.0 + zeta2 * zeta2 * zeta3_m2 * zeta23 + (zeta2 * zeta23 * zeta23 - zeta0) * log(1.0 - zeta3));
    // hard chain (:63-65)
    S c = zeta2 * zeta3_m2;
    for (int i = 0; i < nc; i++) {
        S g = zeta3_m1 + d[i] * c * 1.5 - d[i] * d[i] * c * c * (zeta3 - 1.0) * 0.5;
        phi = phi - rho[i] * (m[i] - 1.0) * log(g);
    }
    // dispersion (:69-106), no k_ij for nc != 2
    S mbar(0.0);
    for (int i = 0; i < nc; i++) mbar = mbar + (rho[i] / rho_sum) * m[i];
    S rho1mix(0.0), rho2mix(0.0);
    for (int i = 0; i < nc; i++)
        for (int j = 0; j < nc; j++) {
            S eps_ij = mixn_lift<S, P>(sqrt(eps[i] * eps[j])) / T;
            P s = 0.5 * (sigma[i] + sigma[j]);
            S rhoij = rho[i] * rho[j] * (m[i] * m[j] * (s * s * s)) * eps_ij;
            rho1mix = rho1mix + rhoij;
            rho2mix = rho2mix + rhoij * eps_ij;
        }
    S I1(0.0), I2(0.0);
    S m1 = (mbar - 1.0) / mbar;
    S m2 = m1 * (mbar - 2.0) / mbar;
    for (int i = 0; i < 7; i++) {
        I1 = I1 + (m2 * A2[i] + m1 * A1[i] + A0[i]) * etas[i];
        I2 = I2 + (m2 * B2[i] + m1 * B1[i] + B0[i]) * etas[i];
    }
    S C1 = 1.0 / (1.0 + mbar * (8.0 * zeta3 - 2.0 * zeta3_2) * zeta3_m2 * zeta3_m2 +
                  (1.0 - mbar) * (20.0 * zeta3 - 27.0 * zeta3_2 + 12.0 * zeta3_2 * zeta3 - 2.0 * zeta3_2 * zeta3_2) /
                      ((1.0 - zeta3) * (1.0 - zeta3) * (2.0 - zeta3) * (2.0 - zeta3)));
    phi = phi + (-1.0 * rho1mix * 2.0 * I1 - rho2mix * C1 * I2 * mbar) * PI;
    // dipoles (:156-208)
    bool dipolar = false;
    for (int i = 0; i < nc; i++) dipolar = dipolar || re(mu2[i]) > 0.0;
    if (dipolar) {
        S mu2_term[MIXN_MAX];
        for (int i = 0; i < nc; i++) mu2_term[i] = mixn_lift<S, P>(sigma[i] * sigma[i] * sigma[i] * eps[i] * mu2[i]) / T;  // :163
        S phi2(0.0), phi3(0.0);
        for (int i = 0; i < nc; i++)
            for (int j = i; j < nc; j++) {
                P s_ij = 0.5 * (sigma[i] + sigma[j]);
                P mij = sqrt(clamp2(m[i]) * clamp2(m[j]));
                S mij1 = mixn_lift<S, P>((mij - 1.0) / mij);
                S mij2 = mij1 * ((mij - 2.0) / mij);
                S eps_ij_t = mixn_lift<S, P>(sqrt(eps[i] * eps[j])) / T;
                double cc = (i == j) ? 1.0 : 2.0;
                phi2 = phi2 - rho[i] * rho[j] * mu2_term[i] * mu2_term[j] * pair_integral(mij1, mij2, etas, eps_ij_t) / (s_ij * s_ij * s_ij) * cc;
                for (int k = j; k < nc; k++) {
                    P sij = 0.5 * (sigma[i] + sigma[j]), sik = 0.5 * (sigma[i] + sigma[k]), sjk = 0.5 * (sigma[j] + sigma[k]);
                    P mijk = cbrt(clamp2(m[i]) * clamp2(m[j]) * clamp2(m[k]));
                    S mijk1 = mixn_lift<S, P>((mijk - 1.0) / mijk);
                    S mijk2 = mijk1 * ((mijk - 2.0) / mijk);
                    int distinct = 1 + (j != i) + (k != j);
                    double c3 = (distinct == 1) ? 1.0 : (distinct == 2 ? 3.0 : 6.0);
                    phi3 = phi3 - rho[i] * rho[j] * rho[k] * mu2_term[i] * mu2_term[j] * mu2_term[k] * triplet_integral(mijk1, mijk2, etas) / (sij * sik * sjk) * c3;
                }
            }
        phi2 = phi2 * PI;
        phi3 = phi3 * (4.0 / 3.0 * PI * PI);
        if (re(phi2) == 0.0) phi = phi + phi2;  // 0/0 where no polar component is present (see pcsaft_mix.hpp)
        else phi = phi + phi2 * phi2 / (phi2 - phi3);
    }
    // association (:118-152): one associating component -> phi_self_assoc (:210-239); more -> binary only
    int associating = 0, self_assoc = 0;
    for (int i = 0; i < nc; i++) {
        const P* p = par + 8 * i;
        associating += (re(p[6]) + re(p[7]) != 0.0);
        self_assoc += (re(p[6]) * re(p[7]) != 0.0);
    }
    if (associating > 1) { ok = false; return phi; }
    if (associating == 1 && self_assoc == 1) {
        P kap(0.0), eab(0.0), na_sum(0.0), sg(0.0);
        S dd(0.0), rhoa(0.0), rhob(0.0);
        for (int i = 0; i < nc; i++) {
            const P* p = par + 8 * i;
            kap = kap + p[4]; eab = eab + p[5]; na_sum = na_sum + p[6]; sg = sg + p[6] * sigma[i];
            dd = dd + d[i] * p[6];
            rhoa = rhoa + rho[i] * p[6];
            rhob = rhob + rho[i] * p[7];
        }
        sg = sg / na_sum;
        dd = dd * (1.0 / na_sum);
        // association_strength(0, 0, ...) (:500-522) with the site-weighted sigma and d
        S k = dd * dd / (dd + dd) * zeta2 * zeta3_m1;
        S delta = zeta3_m1 * (k * (2.0 * k + 3.0) + 1.0) * (sg * sg * sg * kap) * (exp(mixn_lift<S, P>(eab) / T) - 1.0);
        S xa, xb;
        site_fractions_two_types(rhoa, rhob, delta, xa, xb);  // :235-238
        phi = phi + rhoa * site_f(xa) + rhob * site_f(xb);
    }
    return phi;
}

// :395-420 for nc components: a, p, mu[nc], v[nc].  F is the number type of the state (double, long double, or a DualN of
// one of them whose tangents are the directions of a gradient); P = double: plain parameters, P = F: parameters that carry
// tangents like the state.
template <class F, class P>
bool derivatives_mixn(int nc, const P* par, F T, const F* rho, F& a, F& p, F* mu, F* v) {
    typedef HyperDual<F, MIXN_MAX + 1> H;
    auto lift = [](F x) { H h; h.re = x; return h; };
    H volume = lift(F(1));
    volume.eps1[nc] = F(1);
    volume.eps2 = F(1);
    H dens[MIXN_MAX];
    F rs = 0;
    for (int i = 0; i < nc; i++) {
        H moles = lift(rho[i]);
        moles.eps1[i] = F(1);
        dens[i] = moles / volume;
        rs = rs + rho[i];
    }
    bool ok;
    H A;
    if constexpr (std::is_same<P, double>::value) {
        A = helmholtz_energy_density_mixn<H>(nc, par, lift(T), dens, ok) * volume;
    } else {
        static_assert(std::is_same<P, F>::value, "parameters are plain doubles or of the state's type");
        H parh[8 * MIXN_MAX];
        for (int k = 0; k < 8 * nc; k++) parh[k] = lift(par[k]);
        A = helmholtz_energy_density_mixn<H, H>(nc, parh, lift(T), dens, ok) * volume;
    }
    p = rs - A.eps2;
    for (int i = 0; i < nc; i++) {
        mu[i] = A.eps1[i];
        v[i] = -(F(1) - A.eps1eps2[i]) / (-rs - A.eps1eps2[nc]);
    }
    a = A.re;
    return ok;
}

}  // namespace oracle
