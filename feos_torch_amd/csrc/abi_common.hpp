// Shared helpers of the C-ABI translation units (error string, argument checks).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

namespace pcs_abi {

extern thread_local char g_err[256];  // defined in pure_kernels.hip; read through pcs_last_error()

inline int fail(const char* what, hipError_t e) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return 1;
}
inline int fail_msg(const char* what) {
    snprintf(g_err, sizeof(g_err), "%s", what);
    return 2;
}
inline int fail_msg(const char* entry, const char* what) {  // "<entry>: <what>"
    snprintf(g_err, sizeof(g_err), "%s: %s", entry, what);
    return 2;
}
inline int check_n(int64_t n) {
    if (n < 0) return fail_msg("n must be >= 0");
    if (n >= (int64_t)1 << 31) return fail_msg("n must be < 2^31 rows per call (shard larger batches)");
    return 0;
}
inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Start of every entry point: clears the error string and checks n and the required pointers (the caller spells them out:
// `params && temp && ...`).  GO_ON: launch; anything else is the entry point's return value (0 for an empty batch).
constexpr int GO_ON = -1;
inline int enter(int64_t n, bool required_present, const char* null_message) {
    g_err[0] = 0;
    if (int e = check_n(n)) return e;
    if (n == 0) return 0;
    if (!required_present) return fail_msg(null_message);
    return GO_ON;
}

// 0, or the error "<entry>: <what> must be 16-byte aligned" when one of the pointers is not (the kernels move parameter and
// gradient rows as double2; a null pointer passes)
template <class... P>
inline int aligned16(const char* entry, const char* what, const P*... ptrs) {
    if (((reinterpret_cast<uintptr_t>(ptrs) | ...) & 15) == 0) return 0;
    snprintf(g_err, sizeof(g_err), "%s: %s must be 16-byte aligned", entry, what);
    return 2;
}

// End of every launch sequence: 0, or the pending launch error under the name `what`
inline int launched(const char* what) {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(what, e);
}

// workgroups of `block` lanes that cover n rows
inline unsigned grid_for(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }

// Launch functions the entry points of pure_kernels.hip call in units built with other flags (feos_torch_amd/build.py).
// pure_robust.hip, strict IEEE semantics: stage 2 of the VLE (k_pure_vle_robust)
int launch_pure_vle_retry(const double* params, const double* temp, double* p_sat, double* rho_eq, double* rho_vl,
                          uint8_t* status, int32_t* iters, const int32_t* retry, int64_t n, hipStream_t s);
// pure_fp64.hip, no re-association: the all-fp64 VLE kernel k_pure_vle<false> and k_pure_liquid_density
int launch_pure_vle_full(const double* params, const double* temp, int64_t n, double* p_sat, double* rho_eq, double* rho_vl,
                         uint8_t* status, int32_t* iters, int32_t* retry, hipStream_t s);
int launch_pure_liquid_density(const double* params, const double* temp, const double* pressure, int64_t n, double* rho_out,
                               double* rho_root, uint8_t* status, hipStream_t s);

// Device-side counters (retry-list count, work-queue control block) are zeroed by a KERNEL on the call's stream, not by
// hipMemsetAsync: every operation of a call is then a kernel node of a hipGraph capture.  What round 2's one A/B run shows
// (profiles/r02_capture_ab.log, scripts/dev/capture_ab.py plants a stale count of 0x7FFFFFF0 before every replay): with this
// reset a capture of pcs_pure_vle replayed behind pending launches is bit-identical to the eager call 3/3 times; with the
// hipMemsetAsync reset of round 1 the second replay ended in a GPU memory access fault.  The log does not say which access
// faulted.  The reading that fits the code: the replayed memset was not reliably ordered before / visible to the first
// kernel, and the list PRODUCERS of that build appended without a bound (retry[1 + atomicAdd(&retry[0], 1)] = i), i.e. ~8 GB
// past the workspace on the planted count.  Since round 3 every producer bounds its slot by n (pure_kernels.hip,
// mix_kernels.hip, gc_kernels.hip) like the consumers always did, so a stale or foreign counter can no longer send a store
// out of the list whatever resets it.
template <int DUMMY = 0>
__global__ void k_zero_ints(int32_t* __restrict__ p, int count) {
    for (int k = threadIdx.x; k < count; k += blockDim.x) p[k] = 0;
}
inline int zero_ints(int32_t* p, int count, hipStream_t s) {
    hipLaunchKernelGGL(k_zero_ints<0>, dim3(1), dim3(64), 0, s, p, count);
    return launched("k_zero_ints launch");
}

}  // namespace pcs_abi
