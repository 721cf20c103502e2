// block_scan.h — the workgroup prefix scan of the count / scan / fill post-passes (graph_pack.hip, molfile.hip): one
// definition (internal).
#pragma once
#include <hip/hip_runtime.h>

namespace mnx {

// Exclusive prefix sum of one value per thread over a workgroup of NT threads (Hillis-Steele in LDS, two buffers); *total
// receives the sum. buf holds 2 * NT words. Ends with a barrier, so it may be called again at once.
template <int NT>
__device__ __forceinline__ unsigned block_scan_excl(unsigned v, unsigned* buf, unsigned* total) {
    const int tid = threadIdx.x;
    int cur = 0;
    buf[tid] = v;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {
        const unsigned x = buf[cur * NT + tid] + (tid >= d ? buf[cur * NT + tid - d] : 0u);
        buf[(cur ^ 1) * NT + tid] = x;
        cur ^= 1;
        __syncthreads();
    }
    const unsigned incl = buf[cur * NT + tid];
    *total = buf[cur * NT + NT - 1];
    __syncthreads();
    return incl - v;
}

}  // namespace mnx
