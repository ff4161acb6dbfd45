// Class-uniform waves: the workgroup counting sort every bucketed kernel orders its rows with.
#pragma once
#include <hip/hip_runtime.h>

namespace pcs {

// bins[0..NBINS) = 0.  Ends WITHOUT a barrier: the caller's next __syncthreads() -- the one its parameter staging pays
// anyway in the pure kernels -- must come before block_order_sort.
template <int NBINS>
__device__ __forceinline__ void block_order_reset(int* bins) {
    if (threadIdx.x < NBINS) bins[threadIdx.x] = 0;
}

// LDS counting sort of the workgroup's lanes by key() in [0, NBINS): afterwards perm[0..blockDim.x) lists the lanes bucket
// by bucket (the order inside a bucket is whatever the atomics give: irrelevant, rows are independent) and lane t works on
// the row of lane perm[t].  bins must be zero and that visible (block_order_reset + a barrier); every lane of the
// workgroup makes the call.  Three barriers, the last one after perm is complete.  The key is a callable so that it is
// computed here, behind the caller's barrier, e.g. from rows staged in LDS; a kernel with a ragged last block gives its
// lanes past n a bucket of their own at the end (NBINS = classes + 1).  Callers capture by value ([=]): with a capture
// by reference the generated code of k_gc_bubble_dew differed from the written-out sort, by value it is identical.
template <int NBINS, class Key>
__device__ __forceinline__ void block_order_sort(int* bins, int* perm, Key key_of_lane) {
    const int t = threadIdx.x;
    const int key = key_of_lane();
    atomicAdd(&bins[key], 1);
    __syncthreads();
    if (t == 0) {
        int acc = 0;
#pragma unroll
        for (int b = 0; b < NBINS; b++) {
            int c = bins[b];
            bins[b] = acc;
            acc += c;
        }
    }
    __syncthreads();
    perm[atomicAdd(&bins[key], 1)] = t;
    __syncthreads();
}

// reset + barrier + sort, for kernels without a staging barrier to share
template <int NBINS, class Key>
__device__ __forceinline__ void block_order(int* bins, int* perm, Key key_of_lane) {
    block_order_reset<NBINS>(bins);
    __syncthreads();
    block_order_sort<NBINS>(bins, perm, key_of_lane);
}

}  // namespace pcs
