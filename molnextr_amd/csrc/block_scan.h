// block_scan.h — the workgroup prefix scan of the count / scan / fill post-passes (graph_pack.hip, molfile.hip, smiles.hip,
// expand.hip) and the scans of the text and table writers over their molecules: one definition (internal). What the text writers share in front of
// their scans, per molecule, is in atom_symbol.h.
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
// lengths in tiles of TEXT_SCAN_THREADS with a running 64-bit carry, by ONE workgroup (graph_pack.hip's scan over the images,
// on one column); a total beyond 2^32 - 1 saturates and sets totals[1].
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

constexpr int MOL_SCAN_THREADS = 1024;

// atom0 / bond0 / text0 of every record of a table writer (mnx_graph_pack, mnx_expand_pack): an exclusive scan of n_atoms, n_bonds
// and smiles_len over the molecules in tiles of MOL_SCAN_THREADS with a running carry, by ONE workgroup (n molecules are a few
// thousand words). 64-bit carries: a total beyond 2^32 - 1 saturates and sets totals[3].
static __global__ __launch_bounds__(MOL_SCAN_THREADS) void mol_scan_kernel(mnx_mol* __restrict__ mols, int n, unsigned atom_cap,
                                                                           unsigned bond_cap, unsigned text_cap,
                                                                           unsigned* __restrict__ totals) {
    __shared__ unsigned scan[2 * MOL_SCAN_THREADS];
    const int tid = threadIdx.x;
    unsigned long long ca = 0, cb = 0, ct = 0;
    for (int base = 0; base < n; base += MOL_SCAN_THREADS) {
        const int b = base + tid;
        const unsigned a = b < n ? mols[b].n_atoms : 0u, bo = b < n ? mols[b].n_bonds : 0u, t = b < n ? mols[b].smiles_len : 0u;
        unsigned ta, tb, tt;
        const unsigned ea = block_scan_excl<MOL_SCAN_THREADS>(a, scan, &ta);
        const unsigned eb = block_scan_excl<MOL_SCAN_THREADS>(bo, scan, &tb);
        const unsigned et = block_scan_excl<MOL_SCAN_THREADS>(t, scan, &tt);
        if (b < n) {
            mols[b].atom0 = (unsigned)min(ca + ea, 0xffffffffull);
            mols[b].bond0 = (unsigned)min(cb + eb, 0xffffffffull);
            mols[b].text0 = (unsigned)min(ct + et, 0xffffffffull);
        }
        ca += ta; cb += tb; ct += tt;
    }
    if (tid == 0) {
        totals[0] = (unsigned)min(ca, 0xffffffffull);
        totals[1] = (unsigned)min(cb, 0xffffffffull);
        totals[2] = (unsigned)min(ct, 0xffffffffull);
        totals[3] = (ca > atom_cap || cb > bond_cap || ct > text_cap) ? 1u : 0u;
    }
}

}  // namespace mnx
