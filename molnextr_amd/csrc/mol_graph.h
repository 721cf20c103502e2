// mol_graph.h — the neighbour lists of one packed molecule in LDS, built by one workgroup: what canon_rank_kernel and
// smiles_kernel (smiles.hip) and fingerprint_kernel (fingerprint.hip) begin with, stated once (internal). Atom a's list is
// lst[off[a] .. off[a + 1]): one entry (path_search.h: neighbour, class or word, owner) per bond record at either end, in no
// fixed order. Every array is the caller's: this header declares no __shared__ storage. The pieces run in the order they
// stand in, each by all MG_THREADS threads; a caller keeps its own votes, refusals and record between them. The LDS atomics
// count degrees and hand out the slots of lists that every caller sorts by value or walks as a set: none decides a result.
#pragma once
#include "atom_symbol.h"
#include "block_scan.h"
#include "path_search.h"

namespace mnx {

constexpr int MG_THREADS = 256, MG_MAX = 1024;           // a workgroup; atoms held in LDS (999 at most)
constexpr int MG_PER = MG_MAX / MG_THREADS;              // neighbouring atoms per thread in the scan
constexpr int MG_SLOTS = 2 * MG_MAX;                     // neighbour-list entries: two per bond (999 bonds at most)
static_assert(MG_PER * MG_THREADS == MG_MAX && MG_MAX > 999 && MG_SLOTS >= 2 * 999, "every admitted molecule fits");
static_assert(MG_MAX == 1 << paths::ENTRY_ATOM_BITS, "an atom index fills the neighbour and owner fields of an entry");
using paths::entry, paths::entry_nbr, paths::entry_owner, paths::entry_word;

// Degrees: cnt[a] += 1 at both ends of every good record; per_bond(k, i, j) sees each good record once. Returns whether one of
// this thread's records is BAD: i or j is no atom of the molecule, or i == j. In front: cnt[0 .. MG_MAX) cleared, a barrier.
// Behind: none — the caller's vote on the flag (__syncthreads_or) is the barrier graph_lists needs.
struct NoBondHook { __device__ void operator()(int, unsigned, unsigned) const {} };
template <typename PerBond = NoBondHook>
__device__ __forceinline__ int graph_degrees(const Molecule& mol, unsigned* cnt, PerBond per_bond = {}) {
    int bad = 0;
    for (int k = threadIdx.x; k < (int)mol.m.n_bonds; k += MG_THREADS) {
        const unsigned i = mol.B[k].i, j = mol.B[k].j;
        if (i >= mol.m.n_atoms || j >= mol.m.n_atoms || i == j) { bad = 1; continue; }
        per_bond(k, i, j);
        atomicAdd(&cnt[i], 1u);                           // a count does not depend on the order of its increments
        atomicAdd(&cnt[j], 1u);
    }
    return bad;
}

// Lists: off[0 .. MG_MAX] from a scan of the degrees, MG_PER neighbouring atoms per thread, off[MG_MAX] the number of entries;
// then every record takes a slot, any free one, in the list of either end. word(k) is the class field of both entries of
// record k; own(k, end) the caller's own bits, from paths::ENTRY_BITS up, of its entry in the list of i (end 0) or of j (end
// 1). scan: 2 * MG_THREADS words; cnt ends as the degrees again. In front: a barrier behind graph_degrees, no record bad.
// Behind: a barrier.
struct NoOwnBits { __device__ unsigned operator()(int, int) const { return 0u; } };
template <typename Word, typename Own = NoOwnBits>
__device__ __forceinline__ void graph_lists(const Molecule& mol, unsigned* cnt, unsigned* off, unsigned* scan, unsigned* lst, Word word,
                                            Own own = {}) {
    const int tid = threadIdx.x;
    unsigned d[MG_PER], sum = 0, total;
#pragma unroll
    for (int q = 0; q < MG_PER; ++q) { d[q] = cnt[MG_PER * tid + q]; sum += d[q]; }
    unsigned e = block_scan_excl<MG_THREADS>(sum, scan, &total);
#pragma unroll
    for (int q = 0; q < MG_PER; ++q) { off[MG_PER * tid + q] = e; cnt[MG_PER * tid + q] = 0; e += d[q]; }
    if (tid == 0) off[MG_MAX] = total;
    __syncthreads();
    for (int k = tid; k < (int)mol.m.n_bonds; k += MG_THREADS) {
        const unsigned i = mol.B[k].i, j = mol.B[k].j, w = word(k);
        lst[off[i] + atomicAdd(&cnt[i], 1u)] = entry(j, w, i) | own(k, 0);
        lst[off[j] + atomicAdd(&cnt[j], 1u)] = entry(i, w, j) | own(k, 1);
    }
    __syncthreads();
}

// A DUPLICATE PAIR: two entries of one list, at slots u and s, with the same neighbour (n and mine). graph_duplicate: whether
// one of this thread's entries is half of one, the lists as graph_lists left them. In front: graph_lists' barrier. Behind:
// none — the caller votes.
__device__ __forceinline__ bool graph_twice(unsigned n, unsigned u, unsigned mine, unsigned s) { return n == mine && u != s; }
__device__ __forceinline__ int graph_duplicate(const Molecule& mol, const unsigned* off, const unsigned* lst) {
    int dup = 0;
    for (int s = threadIdx.x; s < 2 * (int)mol.m.n_bonds; s += MG_THREADS) {
        const unsigned mine = entry_nbr(lst[s]), a = entry_owner(lst[s]);
        for (unsigned u = off[a]; u < off[a + 1]; ++u) dup |= graph_twice(entry_nbr(lst[u]), u, mine, (unsigned)s);
    }
    return dup;
}

}  // namespace mnx
