// tables_out.h — the output side of the table writers (graph_pack.hip, smiles_read.hip, normalize.hip and kekulize.hip through
// respell_pass.h, expand.hip and formula.hip through grow_pass.h, main_mol.hip through select_pass.h), once (internal): how the fields of an atom and a bond record
// lie in their 64-bit words, the capped stores behind an offset, what a count kernel leaves in mnx_mol, the scan over the
// molecules between count and fill, and the three launches. A fill kernel says where a record's fields come from; where they
// go is here. The arenas arrive as a TablesOut (table_types.h). One molecule of a pass from tables to tables is table_pass.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/molnextr_hip.h"
#include "block_scan.h"
#include "table_types.h"

namespace mnx {

// ---- the record layouts of molnextr_hip.h as whole 64-bit words (little endian), padding bytes zero ----
//   atom word 0: sym0 | sym_len << 32 | index << 48     word 1: x_bin | y_bin << 16     word 2: score
//   bond word 0: i | j << 16 | type << 32 | rev << 40   word 1: score
static_assert(sizeof(mnx_mol) == 40 && sizeof(mnx_atom) == 24 && sizeof(mnx_bond) == 16 && sizeof(mnx_read) == 16,
              "record layout of molnextr_hip.h");
static_assert(offsetof(mnx_atom, sym0) == 0 && offsetof(mnx_atom, sym_len) == 4 && offsetof(mnx_atom, index) == 6 &&
              offsetof(mnx_atom, x_bin) == 8 && offsetof(mnx_atom, y_bin) == 10 && offsetof(mnx_atom, score) == 16,
              "atom_word0 / atom_word1 spell mnx_atom");
static_assert(offsetof(mnx_bond, i) == 0 && offsetof(mnx_bond, j) == 2 && offsetof(mnx_bond, type) == 4 &&
              offsetof(mnx_bond, rev) == 5 && offsetof(mnx_bond, score) == 8, "bond_word0 spells mnx_bond");

__device__ __forceinline__ unsigned long long atom_word0(unsigned sym0, unsigned sym_len, unsigned index) {
    return (unsigned long long)sym0 | (unsigned long long)(sym_len & 0xffffu) << 32 | (unsigned long long)(index & 0xffffu) << 48;
}
__device__ __forceinline__ unsigned long long atom_word1(unsigned x_bin, unsigned y_bin) {
    return (unsigned long long)(x_bin & 0xffffu) | (unsigned long long)(y_bin & 0xffffu) << 16;
}
__device__ __forceinline__ unsigned long long bond_word0(unsigned i, unsigned j, unsigned type, unsigned rev) {
    return (unsigned long long)(i & 0xffffu) | (unsigned long long)(j & 0xffffu) << 16 | (unsigned long long)(type & 0xffu) << 32 |
           (unsigned long long)(rev & 0xffu) << 40;
}
__device__ __forceinline__ unsigned long long score_word(double score) { return (unsigned long long)__double_as_longlong(score); }
// for a writer that passes fields of an input record through (expand.hip): the bits of `index`, of the two bins, of a bond's fields
constexpr unsigned long long ATOM_INDEX_BITS = 0xffff000000000000ull, ATOM_BINS_BITS = 0xffffffffull, BOND_FIELD_BITS = 0xffffffffffffull;

// ---- capped stores: record `at` of the arena (byte `at` of the text), compared in 64 bits; nothing at or beyond a capacity ----
__device__ __forceinline__ bool put_atom(const TablesOut& o, unsigned long long at, unsigned long long w0, unsigned long long w1,
                                         unsigned long long w2) {
    if (at >= o.atom_cap) return false;
    unsigned long long* r = o.atoms + at * 3;
    r[0] = w0;
    r[1] = w1;
    r[2] = w2;
    return true;
}
__device__ __forceinline__ void put_bond(const TablesOut& o, unsigned long long at, unsigned long long w0, unsigned long long w1) {
    if (at >= o.bond_cap) return;
    o.bonds[at * 2] = w0;
    o.bonds[at * 2 + 1] = w1;
}
__device__ __forceinline__ void put_text(const TablesOut& o, unsigned long long at, const unsigned char* src, unsigned n) {
    for (unsigned c = 0; c < n; ++c)
        if (at + c < o.text_cap) o.text[at + c] = (char)src[c];
}

// what count leaves of a molecule: everything of the record but atom0 / bond0 / text0, which are the scan's
__device__ __forceinline__ void store_mol_counts(mnx_mol* m, unsigned n_atoms, unsigned n_bonds, unsigned smiles_len,
                                                 unsigned flags, double overall) {
    m->n_atoms = n_atoms;
    m->n_bonds = n_bonds;
    m->smiles_len = smiles_len;
    m->flags = flags;
    m->reserved = 0;
    m->overall_score = overall;
}

constexpr int MOL_SCAN_THREADS = 1024;

// atom0 / bond0 / text0 of every record of a table writer: an exclusive scan of n_atoms, n_bonds and smiles_len over the molecules
// in tiles of MOL_SCAN_THREADS with a running carry, by ONE workgroup (n molecules are a few thousand words). 64-bit carries: a
// total beyond 2^32 - 1 saturates and sets totals[3].
static __global__ __launch_bounds__(MOL_SCAN_THREADS) void mol_scan_kernel(const TablesOut o, int n, unsigned* __restrict__ totals) {
    __shared__ unsigned scan[2 * MOL_SCAN_THREADS];
    mnx_mol* __restrict__ mols = o.mols;
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
        totals[3] = (ca > o.atom_cap || cb > o.bond_cap || ct > o.text_cap) ? 1u : 0u;
    }
}

// The three launches of a table writer whose count and fill kernels take the same arguments, one workgroup of `threads` per
// molecule: count, the scan over the n molecules, fill.
template <typename Count, typename Fill, typename... Args>
hipError_t count_scan_fill(Count count_kernel, Fill fill_kernel, int n, int threads, const TablesOut& o, unsigned* totals,
                           hipStream_t s, Args... args) {
    hipLaunchKernelGGL(count_kernel, dim3(n), dim3(threads), 0, s, args...);
    hipLaunchKernelGGL(mol_scan_kernel, dim3(1), dim3(MOL_SCAN_THREADS), 0, s, o, n, totals);
    hipLaunchKernelGGL(fill_kernel, dim3(n), dim3(threads), 0, s, args...);
    return hipGetLastError();
}

}  // namespace mnx
