// Host restatement of the two fp64 refinements of csrc/dual.hpp (pure-component unit): the third-order reciprocal step
// (PCS_FAST_RCP == 1) and the coupled square-root refinement (PCS_FAST_SQRT), in plain C++ with std::fma.  The hardware
// seeds v_rcp_f64 / v_rsq_f64 do not exist on the host: the seed is the exact value times (1 + delta) with an INJECTED
// relative error delta, |delta| <= 2^-22 (twice the loosest bound the ISA text gives the estimates), random of both signs
// plus the two extreme values.  Arguments: N_LOG log-uniform in 1e-300 .. 1e300 and N_POW2 in [1, 2) next to the powers of
// two.  The reference is the long-double quotient / square root; the error is counted in ulps of the double result.
// Prints the maxima and exits 1 if a reciprocal is more than 1 ulp or a square root more than 2 ulp off, or if a special
// argument (0, subnormal, inf, NaN; negative for the square root) comes out as a finite number.
//   usage: fast_math_check [n_log [n_pow2]]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

static_assert(std::numeric_limits<long double>::digits >= 64, "the reference needs an extended long double");

// r0 -> r0 (1 + e + e^2), e = 1 - x r0: error e^3
static double recip_refine(double x, double r0) {
    const double e = std::fma(-x, r0, 1.0);
    const double t = std::fma(e, e, e);
    return std::fma(r0, t, r0);
}

// y0 ~ 1/sqrt(x): g = x y0 ~ sqrt(x), h = y0 / 2 ~ 1/(2 sqrt x); one coupled step on (g, h) with r = 1/2 - g h, then one
// residual correction g += (x - g^2) h
static double sqrt_refine(double x, double y0) {
    double g = x * y0, h = 0.5 * y0;
    const double r = std::fma(-g, h, 0.5);
    g = std::fma(g, r, g);
    h = std::fma(h, r, h);
    return std::fma(std::fma(-g, g, x), h, g);
}

static bool is_positive_normal(double x) { return std::isnormal(x) && x > 0.0; }
// what the device code adds: everything but a positive normal argument gives a quiet NaN (bit test on the argument)
static double sqrt_guarded(double x, double y0) {
    return is_positive_normal(x) ? sqrt_refine(x, y0) : std::numeric_limits<double>::quiet_NaN();
}

static double ulps(double got, long double want) {
    int ex;
    std::frexp((double)want, &ex);                       // want = m 2^ex, m in [0.5, 1)
    const long double ulp = std::ldexp(1.0L, ex - 53);  // spacing of doubles in [2^(ex-1), 2^ex)
    return (double)(std::fabs((long double)got - want) / ulp);
}

// hardware-like estimates of special arguments (v_rcp_f64 / v_rsq_f64 follow IEEE there)
static double rcp_seed_special(double x) { return 1.0 / x; }
static double rsq_seed_special(double x) { return 1.0 / std::sqrt(x); }

int main(int argc, char** argv) {
    const long n_log = argc > 1 ? std::atol(argv[1]) : 1000000, n_pow2 = argc > 2 ? std::atol(argv[2]) : 100000;
    std::vector<double> xs;
    xs.reserve(n_log + n_pow2);
    std::mt19937_64 rng(20260);
    std::uniform_real_distribution<double> expo(-300.0, 300.0), unit(-1.0, 1.0);
    for (long i = 0; i < n_log; i++) xs.push_back(std::pow(10.0, expo(rng)));
    for (long i = 0; i < n_pow2; i++) {  // 1, 1 + ulp, ... and 2 - ulp, 2 - 2 ulp, ...: both sides of a binade boundary
        const long k = i / 2;
        const uint64_t bits = (i % 2 == 0) ? (0x3ff0000000000000ull + (uint64_t)k) : (0x4000000000000000ull - 1 - (uint64_t)k);
        double x;
        std::memcpy(&x, &bits, 8);
        xs.push_back(x);
    }
    const long double dmax = std::ldexp(1.0L, -22);
    double worst_r = 0.0, worst_s = 0.0, at_r = 0.0, at_s = 0.0;
    long bad_r = 0, bad_s = 0, cases = 0;
    for (double x : xs) {
        const long double deltas[3] = {dmax * (long double)unit(rng), dmax, -dmax};
        for (long double d : deltas) {
            for (double sx : {x, -x}) {
                const long double q = 1.0L / (long double)sx;
                const double u = ulps(recip_refine(sx, (double)(q * (1.0L + d))), q);
                if (u > worst_r) worst_r = u, at_r = sx;
                bad_r += !(u <= 1.0);
            }
            const long double s = sqrtl((long double)x);
            const double u = ulps(sqrt_guarded(x, (double)((1.0L / s) * (1.0L + d))), s);
            if (u > worst_s) worst_s = u, at_s = x;
            bad_s += !(u <= 2.0);
            cases++;
        }
    }
    // arguments the solvers must see as failures: never a finite number
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double special[] = {0.0, -0.0, 4.9e-324, -4.9e-324, 1e-310, -1e-310, inf, -inf, nan};
    long finite_special = 0;
    for (double x : special) {
        finite_special += std::isfinite(recip_refine(x, rcp_seed_special(x)));
        finite_special += std::isfinite(sqrt_guarded(x, rsq_seed_special(x)));
    }
    for (double x : {-1.0, -1e-300, -1e300, -2.5}) finite_special += std::isfinite(sqrt_guarded(x, rsq_seed_special(x)));
    std::printf("arguments %ld seeds_per_argument 3 cases %ld\n", (long)xs.size(), cases);
    std::printf("recip max_ulp %.4f at %.17g over_1ulp %ld\n", worst_r, at_r, bad_r);
    std::printf("sqrt max_ulp %.4f at %.17g over_2ulp %ld\n", worst_s, at_s, bad_s);
    std::printf("special finite %ld\n", finite_special);
    return (bad_r || bad_s || finite_special) ? 1 : 0;
}
