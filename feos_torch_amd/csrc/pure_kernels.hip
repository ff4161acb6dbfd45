// gfx950 kernels + C ABI for the pure-component PC-SAFT path (see include/pcsaft_hip.h).  Launch shape and memory handling:
// pure_vle_rows.hpp.
//
// The pure path is three units (feos_torch_amd/build.py), all but the last with the relaxed floating-point flags:
//   pure_kernels.hip  (this file) with -fassociative-math -freciprocal-math: the pressure-only VLE kernels (0.783 -> 0.750 ms
//                     per 1e7 rows, x1.044), the Jacobian kernels (x1.13), fallback, derivatives, their VJP, and the whole C ABI;
//   pure_fp64.hip     without re-association: the all-fp64 VLE kernel and the liquid-density kernel, which it makes slower;
//   pure_robust.hip   strict IEEE semantics: stage 2 of the VLE (k_pure_vle_robust).
// A build-level switch like PCS_FAST_RCP, not an experiment: all units are always built and linked.  The entry points here
// reach the other two through the launch functions declared in abi_common.hpp.
#include "../../include/pcsaft_hip.h"
#include "abi_common.hpp"
#include "pure_vle_rows.hpp"
#include "pure_jacobian.hpp"

using namespace pcs_abi;

thread_local char pcs_abi::g_err[256] = "";

namespace {

constexpr int BLOCK = STAGE_BLOCK;  // workgroup size, padded row and stage_rows: pure_stage.hpp
constexpr int ROW_PAD = STAGE_ROW_PAD;

// the pressure-only kernel handing out rho_vl (pcs_pure_vapor_pressure with densities): p_sat and status bit for bit as
// k_pure_vle<true, false>, the densities of the solved rows through vle_polish_densities
__global__ __launch_bounds__(BLOCK, K1_WAVES_LITE) void k_pure_vle_rho(const double* __restrict__ params,
                                                    const double* __restrict__ temp, int64_t n,
                                                    double* __restrict__ p_sat, double* __restrict__ rho_eq,
                                                    double* __restrict__ rho_vl, uint8_t* __restrict__ status,
                                                    int32_t* __restrict__ iters, int32_t* __restrict__ retry) {
    pure_vle_rows<true, false, true>(params, temp, n, p_sat, rho_eq, rho_vl, status, iters, retry);
}

// the pressure-only kernel on rows in a reusable tile-local order: p_sat, status and the list as k_pure_vle<true, false>
// (the list's entries in another sequence), no counting sort, waves of one class and like pre-solve work from a domain of ORDER_TILE rows
__global__ __launch_bounds__(BLOCK, K1_WAVES_LITE) void k_pure_vle_ordered(const double* __restrict__ params,
                                                    const double* __restrict__ temp, int64_t n,
                                                    double* __restrict__ p_sat, uint8_t* __restrict__ status,
                                                    int32_t* __restrict__ iters, int32_t* __restrict__ retry,
                                                    const int32_t* __restrict__ order) {
    pure_vle_rows<true, false, false, true>(params, temp, n, p_sat, nullptr, nullptr, status, iters, retry, order);
}

// The order k_pure_vle_ordered consumes, in two kernels.  k_pure_order_key: one row per lane in batch order, the fp32
// pre-solve itself (pure_coef_f32 + vle_presolve_f32 with its PreSignature), and into order_out[row] the row's key
// class * ORDER_SUB + order_subkey -- a function of the row alone.  k_pure_row_order: one workgroup per tile of ORDER_TILE
// rows, the tile's keys from order_out into LDS, counting sort there, the tile's permutation written over them;
// order_out[tile] is a permutation of the tile's row indices, the sequence inside a bucket is whatever the LDS atomics give.
// Tile size from the host-permuted ceiling measurement (scripts/dev/tile_order_ab.py): 16384 rows.
constexpr int ORDER_TILE = 16384;
constexpr int ORDER_SUB = 64;  // sub-keys per class
constexpr int ORDER_BINS = K1_BINS * ORDER_SUB;
static_assert(ORDER_TILE % BLOCK == 0 && ORDER_BINS <= BLOCK && ORDER_BINS <= 256, "one key byte per row, one lane per bin");
// Sub-key of a row whose pre-solve succeeded, from the margins of its two stop decisions and not from the counts: rows near a
// threshold sit next to each other, so a row that changes sides when the parameters move spoils the waves around a bin edge
// only (an order on the bare counts is the fastest on the parameters it was built from and slower than the tau order on
// moved ones: profiles/cost_order_step0.json).  With c = max(m_l, m_v), q = m_liq, both held to [2^-5, 2^5]:
//   major = floor(log2(c c)) + 8 in 0..15   (half-octave bins of the second coupled iteration's margin over [2^-4, 2^4])
//   minor = (floor(log2 q) + 4) >> 1 in 0..3 (two-octave bins of the liquid root's margin), running backwards in odd majors
// floor(log2 x) is the exponent field of x: no logarithm, and a host can repeat the key bit for bit.
constexpr int ORDER_MAJOR = 16, ORDER_MINOR = 4;
static_assert(ORDER_MAJOR * ORDER_MINOR == ORDER_SUB, "sub-key = major * ORDER_MINOR + minor");
__device__ __forceinline__ int order_exponent(float x) { return (int)((__float_as_uint(x) >> 23) & 0xffu) - 127; }
__device__ __forceinline__ int order_subkey(const PreSignature& g) {
    const float c = fminf(fmaxf(fmaxf(g.m_l, g.m_v), 0.03125f), 32.0f), q = fminf(fmaxf(g.m_liq, 0.03125f), 32.0f);
    const int major = min(max(order_exponent(c * c) + 8, 0), ORDER_MAJOR - 1);
    const int minor = min(max((order_exponent(q) + 4) >> 1, 0), ORDER_MINOR - 1);
    return major * ORDER_MINOR + ((major & 1) ? ORDER_MINOR - 1 - minor : minor);
}
// RAW (pcs_pure_order_key): also raw[4 row ..] = n_liq | n_cpl << 8 | code << 16 | flags << 24 | usable << 31, then the bits
// of the margins m_liq, m_l, m_v (PreSignature, pure_f32.hpp)
template <bool RAW>
__global__ __launch_bounds__(BLOCK) void k_pure_order_key(const double* __restrict__ params, const double* __restrict__ temp,
                                                          int64_t n, int32_t* __restrict__ key_out, int32_t* __restrict__ raw) {
    const LaneRow row = stage_lane_row(params, n);
    const double T = temp[row.ii];
    PureCoefF f;
    pure_coef_f32(f, row.par, T);
    double rl, rv;
    float dpl, dpv;
    PreSignature sig;
    const bool warm = vle_presolve_f32<true>(f, rl, rv, dpl, dpv, &sig);  // every lane of the wave makes the call
    if (!row.live) return;
    bool usable = warm && is_finite_bits(T) && T > 0.0;
#pragma unroll
    for (int k = 0; k < 8; k++) usable = usable && is_finite_bits(row.par[k]) && (k > 2 || row.par[k] > 0.0);
    key_out[row.i] = k1_bucket(row.par) * ORDER_SUB + (usable ? order_subkey(sig) : ORDER_SUB - 1);
    if constexpr (RAW) {
        int32_t* o = raw + 4 * row.i;
        o[0] = (int32_t)((uint32_t)sig.n_liq | (uint32_t)sig.n_cpl << 8 | (uint32_t)sig.code << 16 | (uint32_t)sig.flags << 24 | (usable ? 0x80000000u : 0u));
        o[1] = __float_as_int(sig.m_liq);
        o[2] = __float_as_int(sig.m_l);
        o[3] = __float_as_int(sig.m_v);
    }
}
__global__ __launch_bounds__(BLOCK) void k_pure_row_order(int64_t n, int32_t* __restrict__ order_out) {
    __shared__ uint8_t keys[ORDER_TILE];
    __shared__ int bins[ORDER_BINS];
    const int t = threadIdx.x;
    const int64_t tile0 = (int64_t)blockIdx.x * ORDER_TILE;
    const int count = (int)min((int64_t)ORDER_TILE, n - tile0);
    if (t < ORDER_BINS) bins[t] = 0;
    __syncthreads();
    for (int j = t; j < count; j += BLOCK) {
        const int key = min(max(order_out[tile0 + j], 0), ORDER_BINS - 1);
        keys[j] = (uint8_t)key;
        atomicAdd(&bins[key], 1);
    }
    __syncthreads();  // every key of the tile is in LDS: order_out[tile] may be overwritten from here on
    int first = 0;    // lane b: where bucket b starts, its own serial sum over the buckets before it (no cheaper than a scan)
    for (int b = 0; b < t && b < ORDER_BINS; b++) first += bins[b];
    __syncthreads();
    if (t < ORDER_BINS) bins[t] = first;
    __syncthreads();
    for (int j = t; j < count; j += BLOCK) order_out[tile0 + atomicAdd(&bins[keys[j]], 1)] = (int32_t)(tile0 + j);
}

// Rows of the list with bit 31 set (no usable fp32 pre-solve): the all-fp64 fast path.  Solved rows keep the
// bit (the robust pass skips them), rows that need the robust pass get it cleared.
constexpr int FALLBACK_GRID = 1024;
__global__ __launch_bounds__(64) void k_pure_vle_fallback(const double* __restrict__ params, const double* __restrict__ temp,
                                                          double* __restrict__ p_sat, double* __restrict__ rho_eq,
                                                          double* __restrict__ rho_vl,
                                                          uint8_t* __restrict__ status, int32_t* __restrict__ iters,
                                                          int32_t* __restrict__ retry, int64_t n) {
    // count and entries are bounded by n: a list that was not produced by the main kernel of THIS launch (stale or
    // uninitialised workspace handed to pcs_pure_vle_retry, a runtime that reorders the launches) must not fault
    const int count = (int)min((int64_t)max(retry[0], 0), n);
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const uint32_t entry = (uint32_t)retry[1 + k];
        if (!(entry & 0x80000000u)) continue;
        const int64_t i = (int64_t)(entry & 0x7fffffffu);
        if (i >= n) continue;
        double par[8];
#pragma unroll
        for (int j = 0; j < 8; j++) par[j] = params[8 * i + j];
        const double T = temp[i];
        VleResult res;
        int st = rho_eq ? vle_fast<false>(par, T, res, 1e-8, TOL_STEP) : vle_fast<false>(par, T, res, TOL_L_P, TOL_V_P, rho_vl != nullptr);
        if (st == ST_OK) {
            if (p_sat) p_sat[i] = res.p_star * T * P_UNIT;
            if (rho_eq) rho_eq[i] = res.rho_l * (1.0 / RHO_UNIT);
            if (rho_vl) {
                rho_vl[2 * i] = res.rho_v;
                rho_vl[2 * i + 1] = res.rho_l;
            }
            if (iters) iters[i] = res.iters;
            status[i] = 0;
        } else {
            retry[1 + k] = (int32_t)i;  // bit 31 cleared: robust pass
        }
    }
}

// ------------------------------------------------------------------------------------------
// derivatives (a, p, dp) at given (T, rho)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_pure_derivatives(const double* __restrict__ params,
                                                            const double* __restrict__ temp,
                                                            const double* __restrict__ rho_in, int64_t n,
                                                            double* __restrict__ a, double* __restrict__ p,
                                                            double* __restrict__ dp) {
    const LaneRow row = stage_lane_row(params, n);
    const int64_t i = row.i, ii = row.ii;
    PureCoef<double> c;
    pure_coef<double>(c, row.par, temp[ii], false);
    Eval e = pure_eval(c, rho_in[ii]);
    if (!row.live) return;
    if (a) a[i] = e.a;
    if (p) p[i] = e.p;
    if (dp) dp[i] = e.dp;
}

// ------------------------------------------------------------------------------------------
// test probe: the evaluation the fp32 liquid root starts from, in its generic and its fixed-eta form
// ------------------------------------------------------------------------------------------
// out[i] = (a, p, dp, mu) of pure_eval_f32(f, start_rho_f32(f)), then the same four of pure_eval_start_f32(f)
__global__ __launch_bounds__(BLOCK) void k_pure_start_probe(const double* __restrict__ params, const double* __restrict__ temp,
                                                            int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    double par[8];
#pragma unroll
    for (int k = 0; k < 8; k++) par[k] = params[8 * i + k];
    PureCoefF f;
    pure_coef_f32(f, par, temp[i]);
    const EvalF g = pure_eval_f32(f, start_rho_f32(f));
    const EvalF s = pure_eval_start_f32(f);
    float* o = out + 8 * i;
    o[0] = g.a; o[1] = g.p; o[2] = g.dp; o[3] = g.mu;
    o[4] = s.a; o[5] = s.p; o[6] = s.dp; o[7] = s.mu;
}

// ------------------------------------------------------------------------------------------
// K4: Jacobian of a property w.r.t. (8 parameters, T, p) at fixed densities
// ------------------------------------------------------------------------------------------
constexpr int K4_WAVES = 2;  // Jacobian kernels: two (256 VGPRs); held to 168 for three they spill inside the DN<9> pass: 0.89 -> 2.24 ms
template <int WHICH>
__global__ __launch_bounds__(BLOCK, K4_WAVES) void k_pure_jacobian(const double* __restrict__ params,
                                                         const double* __restrict__ temp,
                                                         const double* __restrict__ pressure,
                                                         const double* __restrict__ rho_vl, int64_t n,
                                                         double* __restrict__ jac, const double* __restrict__ gout,
                                                         double* __restrict__ grad_params, double* __restrict__ grad_temp,
                                                         double* __restrict__ grad_press, int polish) {
    __shared__ double lds[BLOCK * ROW_PAD];
    const int64_t row0 = (int64_t)blockIdx.x * BLOCK;
    double par[8];
    // class bucketing as in k_pure_vle for the two liquid-density properties (A/B on 1e7 rows: 4.0 -> 3.9 ms and
    // 12.0 -> 8.4 ms; the vapour-pressure Jacobian gets slightly slower with it, 3.5 -> 3.7 ms, and keeps the row order)
    constexpr bool BUCKET = WHICH == 1 || WHICH == 2;  // the boiling-temperature Jacobian (3) is the vapour-pressure one at heart
    __shared__ int perm[BUCKET ? BLOCK : 1];
    __shared__ int bins[K1_BINS];
    const int t = threadIdx.x;
    if (BUCKET) block_order_reset<K1_BINS>(bins);
    stage_rows(params, n, row0, lds, par);
    int src = t;
    if (BUCKET) {
        block_order_sort<K1_BINS>(bins, perm, [=] { return k1_bucket(&lds[t * ROW_PAD]); });
        src = perm[t];
#pragma unroll
        for (int q = 0; q < 8; q++) par[q] = lds[src * ROW_PAD + q];
    }
    const int64_t i = row0 + src;
    const bool live = i < n;
    const int64_t ii = live ? i : n - 1;
    const double T = temp[ii];
    const double p_pa = (WHICH == 1) ? pressure[ii] : 0.0;
    const double rv = rho_vl[2 * ii], rl = rho_vl[2 * ii + 1];
    double g[10];
    pure_jacobian<WHICH>(par, T, p_pa, rv, rl, g, polish != 0);
    if (!live) return;
    // a failed row carries zero densities -> NaNs; the caller masks by status
    if (jac) {
#pragma unroll
        for (int k = 0; k < 10; k++) jac[10 * i + k] = g[k];
    }
    if (gout) {  // vector-Jacobian form (the backward pass of a property): upstream gradient folded in, no [n,10] round trip
        const double w = gout[i];
        if (grad_params) {
            double2* dst = reinterpret_cast<double2*>(grad_params + 8 * i);
#pragma unroll
            for (int k = 0; k < 4; k++) dst[k] = make_double2(w * g[2 * k], w * g[2 * k + 1]);
        }
        if (grad_temp) grad_temp[i] = (WHICH == 3) ? 0.0 : w * g[8];  // 3: T is the output, not an input
        if (grad_press) grad_press[i] = w * g[9];
    }
}

// ------------------------------------------------------------------------------------------
// vector-Jacobian product of (a, p, dp) w.r.t. (8 parameters, T, rho): autograd of PcSaftPure.derivatives / helmholtz_energy
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_pure_derivatives_vjp(const double* __restrict__ params,
                                                                const double* __restrict__ temp,
                                                                const double* __restrict__ rho_in, int64_t n,
                                                                const double* __restrict__ g_a, const double* __restrict__ g_p,
                                                                const double* __restrict__ g_dp,
                                                                double* __restrict__ grad_params, double* __restrict__ grad_temp,
                                                                double* __restrict__ grad_rho) {
    const LaneRow row = stage_lane_row(params, n);
    const int64_t i = row.i, ii = row.ii;
    double g[VJP_DIRS];
    pure_derivatives_vjp(row.par, temp[ii], rho_in[ii], g_a ? g_a[ii] : 0.0, g_p ? g_p[ii] : 0.0, g_dp ? g_dp[ii] : 0.0, g);
    if (!row.live) return;
    if (grad_params) {
#pragma unroll
        for (int k = 0; k < 8; k++) grad_params[8 * i + k] = g[k];
    }
    if (grad_temp) grad_temp[i] = g[8];
    if (grad_rho) grad_rho[i] = g[9];
}

}  // namespace

extern "C" {

int pcs_abi_version(void) { return 120; }  // 103: pcs_pure_vapor_pressure, pcs_compact_* / pcs_expand_rows; 104: pcs_pure_vle_fp64;
                                            // 105: pcs_mix_stability, pcs_gc_stability; 106: pcs_pure_critical_point(_vjp);
                                            // 107: pcs_pure_start_probe; 108: pcs_pure_boiling_temperature, Jacobian selector 3;
                                            // 109: pcs_pure_enthalpy_of_vaporization(_vjp); 110: pcs_mix_bubble_dew_temperature;
                                            // 111: pcs_mix_point_jacobian; 112: pcs_gc_bubble_dew_temperature;
                                            // 113: pcs_gc_point_jacobian, pcs_gc_point_segment_gradient; 114: pcs_mix_density;
                                            // 115: pcs_gc_density; 116: pcs_pure_row_order, pcs_pure_vle_fast_ordered;
                                            // 117: pcs_mix_henry; 118: pcs_gc_pure_vle; 119: pcs_pure_order_key;
                                            // 120: pcs_gc_henry

const char* pcs_last_error(void) { return g_err; }

// retry list of the pure / gc two-pass schedules (n + 1 ints) or row order + control block of the mixture work queue (n + 64)
int64_t pcs_workspace_bytes(int64_t n) { return (int64_t)sizeof(int32_t) * (n + 64); }

// The main kernel of stage 1, and the kinds of entry point that choose among them
enum class VleKernel { LITE, LITE_POLISH, LITE_RHO, FP64, ORDERED };
enum class VleEntry { VLE, FP64, VAPOR_PRESSURE, ORDERED };  // pcs_pure_vle(_fast), _vle_fp64, _vapor_pressure, _vle_fast_ordered

// main kernel (lean: rows without an fp32 pre-solve go to the list with bit 31 set) + all-fp64 fallback kernel.
//  * pressure only: k_pure_vle<true>, densities converged to ~1e-9 inside the kernel (enough for p*, whose error is of
//    second order in them) and not handed out; on rows in the order of pcs_pure_row_order: k_pure_vle_ordered;
//  * pcs_pure_vapor_pressure with densities: k_pure_vle_rho, the same solve and the same p_sat bits + the exact Newton
//    update of vle_polish_densities on the densities it hands out (the fp32-slope iteration leaves rho_V up to 1.9e-6 off);
//  * rho_vl without rho_eq (the Jacobian kernels' input), and everything of pcs_pure_vle_fp64:
//    k_pure_vle<false>, the fp64 D2 iteration from the fp32 pre-solve's start -- one iteration at the pressure
//    tolerances, which leaves rho_V up to 5.9e-9 off, + vle_polish_densities when rho_vl is an output: 0.98 -> 1.35 ms
//    per 1e7 rows for the second D2 evaluation of both phases;
//  * rho_eq requested (tolerance 1e-8 on the liquid step: two D2 iterations of the all-fp64 kernel, 1.55-1.67 ms): the
//    pressure-only kernel + the exact Newton update of vle_lite_finish<true> instead, 1.22 ms (round 3).
static VleKernel vle_main_kernel(VleEntry entry, bool rho_eq, bool rho_vl) {
    if (entry == VleEntry::ORDERED) return VleKernel::ORDERED;  // pressure-only form: the entry point refuses densities
    if (entry == VleEntry::FP64) return VleKernel::FP64;
    if (rho_eq) return VleKernel::LITE_POLISH;
    if (!rho_vl) return VleKernel::LITE;
    return entry == VleEntry::VAPOR_PRESSURE ? VleKernel::LITE_RHO : VleKernel::FP64;
}

// the pcs_pure_vle* family: stage 1 (zero the retry counter, main kernel over all rows, fallback over the list) and / or
// stage 2 (robust pass over the list in the workspace)
enum : int { VLE_STAGE_FAST = 1, VLE_STAGE_RETRY = 2 };
static int pure_vle_stages(int stages, VleEntry entry, const double* params, const double* temp, int64_t n, double* p_sat,
                           double* rho_eq, double* rho_vl, uint8_t* status, int32_t* iters, void* workspace, void* stream,
                           const int32_t* order = nullptr) {
    if (int e = enter(n, params && temp && status && workspace, "pcs_pure_vle: null required pointer"); e != GO_ON) return e;
    int32_t* retry = static_cast<int32_t*>(workspace);
    hipStream_t s = as_stream(stream);
    if (stages & VLE_STAGE_FAST) {
        if (int ez = zero_ints(retry, 1, s)) return ez;
        const dim3 grid(grid_for(n, BLOCK)), block(BLOCK);
        const VleKernel main = vle_main_kernel(entry, rho_eq, rho_vl);
        switch (main) {
            case VleKernel::LITE: hipLaunchKernelGGL((k_pure_vle<true, false>), grid, block, 0, s, params, temp, n, p_sat, rho_eq, rho_vl, status, iters, retry); break;
            case VleKernel::LITE_POLISH: hipLaunchKernelGGL((k_pure_vle<true, true>), grid, block, 0, s, params, temp, n, p_sat, rho_eq, rho_vl, status, iters, retry); break;
            case VleKernel::LITE_RHO: hipLaunchKernelGGL(k_pure_vle_rho, grid, block, 0, s, params, temp, n, p_sat, rho_eq, rho_vl, status, iters, retry); break;
            case VleKernel::ORDERED: hipLaunchKernelGGL(k_pure_vle_ordered, grid, block, 0, s, params, temp, n, p_sat, status, iters, retry, order); break;
            case VleKernel::FP64:
                if (int ef = launch_pure_vle_full(params, temp, n, p_sat, rho_eq, rho_vl, status, iters, retry, s)) return ef;
        }
        hipLaunchKernelGGL(k_pure_vle_fallback, dim3(FALLBACK_GRID), dim3(64), 0, s, params, temp, p_sat, rho_eq, rho_vl, status,
                           iters, retry, n);
        if (int e = launched(main == VleKernel::ORDERED ? "k_pure_vle_ordered launch" : "k_pure_vle launch")) return e;
    }
    if (stages & VLE_STAGE_RETRY) return launch_pure_vle_retry(params, temp, p_sat, rho_eq, rho_vl, status, iters, retry, n, s);
    return 0;
}

int pcs_pure_vle(const double* params, const double* temp, int64_t n, double* p_sat, double* rho_eq,
                 double* rho_vl, uint8_t* status, int32_t* iters, void* workspace, void* stream) {
    return pure_vle_stages(VLE_STAGE_FAST | VLE_STAGE_RETRY, VleEntry::VLE, params, temp, n, p_sat, rho_eq, rho_vl, status, iters,
                           workspace, stream);
}

int pcs_pure_vle_fp64(const double* params, const double* temp, int64_t n, double* p_sat, double* rho_eq,
                      double* rho_vl, uint8_t* status, int32_t* iters, void* workspace, void* stream) {
    return pure_vle_stages(VLE_STAGE_FAST | VLE_STAGE_RETRY, VleEntry::FP64, params, temp, n, p_sat, rho_eq, rho_vl, status, iters,
                           workspace, stream);
}

int pcs_pure_vapor_pressure(const double* params, const double* temp, int64_t n, double* p_sat, double* rho_vl,
                            uint8_t* status, void* workspace, void* stream) {
    return pure_vle_stages(VLE_STAGE_FAST | VLE_STAGE_RETRY, VleEntry::VAPOR_PRESSURE, params, temp, n, p_sat, nullptr, rho_vl, status,
                           nullptr, workspace, stream);
}

int pcs_pure_vle_fast(const double* params, const double* temp, int64_t n, double* p_sat, double* rho_eq,
                      double* rho_vl, uint8_t* status, int32_t* iters, void* workspace, void* stream) {
    return pure_vle_stages(VLE_STAGE_FAST, VleEntry::VLE, params, temp, n, p_sat, rho_eq, rho_vl, status, iters, workspace, stream);
}

int pcs_pure_row_order(const double* params, const double* temp, int64_t n, int32_t* order_out, void* stream) {
    if (int e = enter(n, params && temp && order_out, "pcs_pure_row_order: null required pointer"); e != GO_ON) return e;
    hipLaunchKernelGGL(k_pure_order_key<false>, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, as_stream(stream), params, temp, n, order_out, nullptr);
    hipLaunchKernelGGL(k_pure_row_order, dim3(grid_for(n, ORDER_TILE)), dim3(BLOCK), 0, as_stream(stream), n, order_out);
    return launched("k_pure_row_order launch");
}

int pcs_pure_order_key(const double* params, const double* temp, int64_t n, int32_t* key_out, int32_t* raw_out, void* stream) {
    if (int e = enter(n, params && temp && key_out && raw_out, "pcs_pure_order_key: null required pointer"); e != GO_ON) return e;
    hipLaunchKernelGGL(k_pure_order_key<true>, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, as_stream(stream), params, temp, n, key_out, raw_out);
    return launched("k_pure_order_key launch");
}

// stage 1 of the pressure-only solve on rows in the order of pcs_pure_row_order: reset, k_pure_vle_ordered, fallback
int pcs_pure_vle_fast_ordered(const double* params, const double* temp, int64_t n, double* p_sat, double* rho_eq, double* rho_vl,
                              uint8_t* status, int32_t* iters, void* workspace, const int32_t* order, void* stream) {
    if (int e = enter(n, params && temp && status && workspace && order, "pcs_pure_vle_fast_ordered: null required pointer"); e != GO_ON) return e;
    if (rho_eq || rho_vl) return fail_msg("pcs_pure_vle_fast_ordered", "pressure-only form: rho_eq and rho_vl must be null");
    return pure_vle_stages(VLE_STAGE_FAST, VleEntry::ORDERED, params, temp, n, p_sat, nullptr, nullptr, status, iters, workspace, stream,
                           order);
}

int pcs_pure_vle_retry(const double* params, const double* temp, int64_t n, double* p_sat, double* rho_eq,
                       double* rho_vl, uint8_t* status, int32_t* iters, void* workspace, void* stream) {
    return pure_vle_stages(VLE_STAGE_RETRY, VleEntry::VLE, params, temp, n, p_sat, rho_eq, rho_vl, status, iters, workspace, stream);
}

int pcs_pure_liquid_density(const double* params, const double* temp, const double* pressure, int64_t n,
                            double* rho_out, double* rho_root, uint8_t* status, void* stream) {
    if (int e = enter(n, params && temp && pressure && status, "pcs_pure_liquid_density: null required pointer"); e != GO_ON) return e;
    return launch_pure_liquid_density(params, temp, pressure, n, rho_out, rho_root, status, as_stream(stream));
}

int pcs_pure_derivatives(const double* params, const double* temp, const double* rho, int64_t n, double* a,
                         double* p, double* dp, void* stream) {
    if (int e = enter(n, params && temp && rho, "pcs_pure_derivatives: null required pointer"); e != GO_ON) return e;
    const unsigned grid = grid_for(n, BLOCK);
    hipLaunchKernelGGL(k_pure_derivatives, dim3(grid), dim3(BLOCK), 0, as_stream(stream), params, temp, rho, n, a, p,
                       dp);
    return launched("k_pure_derivatives launch");
}

int pcs_pure_start_probe(const double* params, const double* temp, int64_t n, float* out, void* stream) {
    if (int e = enter(n, params && temp && out, "pcs_pure_start_probe: null required pointer"); e != GO_ON) return e;
    const unsigned grid = grid_for(n, BLOCK);
    hipLaunchKernelGGL(k_pure_start_probe, dim3(grid), dim3(BLOCK), 0, as_stream(stream), params, temp, n, out);
    return launched("k_pure_start_probe launch");
}

int pcs_pure_derivatives_vjp(const double* params, const double* temp, const double* rho, int64_t n, const double* g_a,
                             const double* g_p, const double* g_dp, double* grad_params, double* grad_temp, double* grad_rho,
                             void* stream) {
    if (int e = enter(n, params && temp && rho, "pcs_pure_derivatives_vjp: null required pointer"); e != GO_ON) return e;
    const unsigned grid = grid_for(n, BLOCK);
    hipLaunchKernelGGL(k_pure_derivatives_vjp, dim3(grid), dim3(BLOCK), 0, as_stream(stream), params, temp, rho, n, g_a, g_p,
                       g_dp, grad_params, grad_temp, grad_rho);
    return launched("k_pure_derivatives_vjp launch");
}

// both Jacobian entry points: `entry` names the caller in the messages; jac or (gout, grad_*) select the output form
static int launch_pure_jacobian(const char* entry, int which, const double* params, const double* temp, const double* pressure,
                                const double* rho_vl, int64_t n, double* jac, const double* gout, double* grad_params,
                                double* grad_temp, double* grad_pressure, hipStream_t s) {
    const int polish = (which & PCS_JAC_POLISH) ? 1 : 0;
    which &= ~PCS_JAC_POLISH;
    if (which == 1 && !pressure) return fail_msg(entry, "pressure required for liquid_density");
    if (int e = aligned16(entry, "grad_params", grad_params)) return e;
    const unsigned grid = grid_for(n, BLOCK);
    switch (which) {
        case 0: hipLaunchKernelGGL(k_pure_jacobian<0>, dim3(grid), dim3(BLOCK), 0, s, params, temp, pressure, rho_vl, n, jac, gout, grad_params, grad_temp, grad_pressure, polish); break;
        case 1: hipLaunchKernelGGL(k_pure_jacobian<1>, dim3(grid), dim3(BLOCK), 0, s, params, temp, pressure, rho_vl, n, jac, gout, grad_params, grad_temp, grad_pressure, polish); break;
        case 2: hipLaunchKernelGGL(k_pure_jacobian<2>, dim3(grid), dim3(BLOCK), 0, s, params, temp, pressure, rho_vl, n, jac, gout, grad_params, grad_temp, grad_pressure, polish); break;
        case 3: hipLaunchKernelGGL(k_pure_jacobian<3>, dim3(grid), dim3(BLOCK), 0, s, params, temp, pressure, rho_vl, n, jac, gout, grad_params, grad_temp, grad_pressure, polish); break;
        default: return fail_msg(entry, "which must be 0, 1, 2 or 3");
    }
    return launched("k_pure_jacobian launch");
}

int pcs_pure_jacobian(int which, const double* params, const double* temp, const double* pressure,
                      const double* rho_vl, int64_t n, double* jac, void* stream) {
    if (int e = enter(n, params && temp && rho_vl && jac, "pcs_pure_jacobian: null required pointer"); e != GO_ON) return e;
    return launch_pure_jacobian("pcs_pure_jacobian", which, params, temp, pressure, rho_vl, n, jac, nullptr, nullptr, nullptr, nullptr,
                                as_stream(stream));
}

int pcs_pure_jacobian_vjp(int which, const double* params, const double* temp, const double* pressure, const double* rho_vl,
                          const double* gout, int64_t n, double* grad_params, double* grad_temp, double* grad_pressure,
                          void* stream) {
    if (int e = enter(n, params && temp && rho_vl && gout, "pcs_pure_jacobian_vjp: null required pointer"); e != GO_ON) return e;
    return launch_pure_jacobian("pcs_pure_jacobian_vjp", which, params, temp, pressure, rho_vl, n, nullptr, gout, grad_params, grad_temp,
                                grad_pressure, as_stream(stream));
}

}  // extern "C"
