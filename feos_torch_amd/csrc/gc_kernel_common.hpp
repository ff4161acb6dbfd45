// Helpers shared by the gc-PC-SAFT translation units (gc_kernels.hip, gc_gradient.hip, gc_temperature.hip, gc_incipient.hip,
// stability_kernels.hip): model struct, LDS staging, class key and row pick (gc_pick_row), entry prologue (gc_enter).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "abi_common.hpp"
#include "block_order.hpp"
#include "gc_model.hpp"

namespace {

using namespace pcs;
using namespace pcs_abi;

template <class P>
struct GcModelT {
    GcCoef<P> c;
    template <class R> PCS_DEV R a(const R& r0, const R& r1) const { return gc_a<P, R>(c, r0, r1); }
    template <class R, class Z> PCS_DEV R a_z(const R& r0, const R& r1, const Z& zeta3) const { return gc_a_z<P, R, Z>(c, r0, r1, zeta3); }
    PCS_DEV double packing(double x0, double x1) const { return x0 * re(c.zk[3][0]) + x1 * re(c.zk[3][1]); }
};

// stage the batch table (S*8 + 3*S*S doubles) into LDS
__device__ __forceinline__ GcTable stage_table(const double* __restrict__ table, int S, double* lds) {
    const int nd = gc_table_doubles(S);
    for (int k = threadIdx.x; k < nd; k += blockDim.x) lds[k] = table[k];
    __syncthreads();
    GcTable tb;
    tb.S = S;
    tb.seg = lds;
    tb.E1 = lds + S * 8;
    tb.E2 = tb.E1 + S * S;
    tb.K = tb.E2 + S * S;
    return tb;
}

// The 80 structure bytes of this lane's row, staged in LDS.  The model set-up (gc_mol) reads single bytes of the row inside its
// loops -- 32 for the molecule sums, up to 2 x 192 in the dispersion double sums, 48 for the bonds -- and as global byte loads
// each of them waits for its own round trip to the cache (one wave per SIMD: nothing hides it).  Lane stride 84 B = 21 dwords
// (odd: conflict-free for equal offsets); the area is lane-private, no barrier needed.  `area` = GC_ROW_LDS_DOUBLES doubles per
// thread of the workgroup.
constexpr int GC_ROW_LDS_STRIDE = 84;
constexpr int GC_ROW_LDS_DOUBLES = 11;
__device__ __forceinline__ const unsigned char* stage_row(const unsigned char* __restrict__ row, double* area) {
    unsigned int* dst = reinterpret_cast<unsigned int*>(reinterpret_cast<unsigned char*>(area) + threadIdx.x * GC_ROW_LDS_STRIDE);
    const uint4* src = reinterpret_cast<const uint4*>(row);
#pragma unroll
    for (int k = 0; k < GC_ROW_BYTES / 16; k++) {
        const uint4 v = src[k];
        dst[4 * k] = v.x; dst[4 * k + 1] = v.y; dst[4 * k + 2] = v.z; dst[4 * k + 3] = v.w;
    }
    return reinterpret_cast<const unsigned char*>(dst);
}

// no-progress leash of the dew-point Newton here (mixture kernels: 20, followed by their damped run): the second pass ends with its
// slowest row; 10 loses no row of the synthetic batch and shortens it: dew 3.70 -> 3.60 ms per 1e6 rows
constexpr int GC_NO_PROGRESS_DEW = 10;

// association class x polarity of a row (the evaluation's branches): key of the workgroup bucketing in the fast pass
constexpr int GC_BINS = 8;
__device__ __forceinline__ int gc_bucket(const unsigned char* __restrict__ row, const GcTable& tb) {
    int associating = 0, self_assoc = 0, polar = 0;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        double ka = 0.0, eab = 0.0, na = 0.0, nb = 0.0, mu2 = 0.0;
#pragma unroll 1
        for (int e = 0; e < GC_MAXE; e++) {
            const int n = row[16 + i * GC_MAXE + e];
            if (n == 0) continue;
            const double* p = tb.seg + 8 * row[i * GC_MAXE + e];
            mu2 += n * p[3] * p[3];
            ka += n * p[4];
            eab += n * p[5];
            na += n * p[6];
            nb += n * p[7];
        }
        associating += (ka * eab != 0.0);
        self_assoc += (na * nb != 0.0);
        polar |= (mu2 > 0.0);
    }
    int cls = 0;
    if (associating == 1 && self_assoc == 1) cls = 1;
    if (associating == 2 && self_assoc == 1) cls = 2;
    if (associating == 2 && self_assoc == 2) cls = 3;
    return 2 * cls + polar;
}

// The row this lane of a BLOCK-thread workgroup works on, or n for none; every lane of the workgroup makes the call and
// comes back (the kernels have barriers of their own behind it).  With `order` (batch-wide class order from the caller,
// computed once per model: the rows are fixed; measured with host-sorted rows: bubble 3.0 -> 2.1 ms, dew 7.8 -> 5.6 ms per
// 1e6 rows) its entry, a foreign one mapped to n: it must not fault.  Without: the rows of the workgroup bucketed by class
// (LDS counting sort), lane t takes the row at sorted position t, so a wave mostly runs one set of branches of the
// evaluation; rows past n sort last, in a bucket of their own.  tb: the table staged in LDS (stage_table).
template <int BLOCK>
__device__ __forceinline__ int64_t gc_pick_row(const unsigned char* __restrict__ rows, const GcTable& tb, int64_t n,
                                               const int32_t* __restrict__ order) {
    const int64_t row0 = (int64_t)blockIdx.x * BLOCK;
    const int64_t i = row0 + threadIdx.x;
    if (order) {
        const int64_t o = i < n ? (int64_t)order[i] : n;
        return (o >= 0 && o < n) ? o : n;
    }
    __shared__ int bins[GC_BINS + 1];
    __shared__ int perm[BLOCK];
    block_order<GC_BINS + 1>(bins, perm, [=] {
        int key = GC_BINS;
        if (i < n) key = gc_bucket(rows + (size_t)i * GC_ROW_BYTES, tb);
        return key;
    });
    const int64_t k = row0 + perm[threadIdx.x];
    return k < n ? k : n;
}

// the one dual-number evaluation site of the gradient kernels, not inlined (register pressure, see mix_jacobian.hpp)
template <class G, class R>
__device__ __attribute__((noinline)) R gc_a_tangent(const GcCoef<G>& c, const R& r0, const R& r1) {
    return gc_a<G, R>(c, r0, r1);
}

constexpr size_t gc_lds_bytes(int S, int block, int per_thread_doubles) {
    return sizeof(double) * ((size_t)(S * 8 + 3 * S * S) + (size_t)per_thread_doubles * block);
}

inline int gc_check(int S, int64_t n) {
    if (int e = check_n(n)) return e;
    if (S < 1 || S > GC_MAXS) return fail_msg("gc: number of segment types must be in [1, 32]");
    return 0;
}

// Start of every gc entry point (abi_common.hpp's enter with the table check): clears the error string, checks n and S, an
// empty batch, the required pointers.  GO_ON: go on (alignment: aligned16); anything else is the entry point's return value.
inline int gc_enter(int S, int64_t n, bool required_present, const char* null_message) {
    g_err[0] = 0;
    if (int e = gc_check(S, n)) return e;
    if (n == 0) return 0;
    if (!required_present) return fail_msg(null_message);
    return GO_ON;
}

}  // namespace
