// block_scan.h — the workgroup prefix scan of the count / scan / fill post-passes (graph_pack.hip, molfile.hip, smiles.hip,
// expand.hip, smiles_read.hip) and the scan of the text writers over their molecules: one definition (internal). What the text
// writers share in front of their scans, per molecule, is in atom_symbol.h; the scan of the table writers over their molecules
// stands with the rest of their output side in tables_out.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/molnextr_hip.h"

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

constexpr int TEXT_SCAN_THREADS = 1024;

// text0 of every record of a text writer (mnx_molfile, mnx_smiles: both begin with text0, len): an exclusive scan of the
// lengths in tiles of TEXT_SCAN_THREADS with a running 64-bit carry, by ONE workgroup (the table writers' scan over their
// molecules, tables_out.h, on one column); a total beyond 2^32 - 1 saturates and sets totals[1].
template <typename Rec>
__global__ __launch_bounds__(TEXT_SCAN_THREADS) void text_scan_kernel(Rec* __restrict__ recs, int n, unsigned out_cap,
                                                                      unsigned* __restrict__ totals) {
    __shared__ unsigned scan[2 * TEXT_SCAN_THREADS];
    const int tid = threadIdx.x;
    unsigned long long carry = 0;
    for (int base = 0; base < n; base += TEXT_SCAN_THREADS) {
        const int b = base + tid;
        unsigned t;
        const unsigned e = block_scan_excl<TEXT_SCAN_THREADS>(b < n ? recs[b].len : 0u, scan, &t);
        if (b < n) recs[b].text0 = (unsigned)min(carry + e, 0xffffffffull);
        carry += t;
    }
    if (tid == 0) {
        totals[0] = (unsigned)min(carry, 0xffffffffull);
        totals[1] = carry > out_cap ? 1u : 0u;
    }
}

}  // namespace mnx
