// match.hip — substructure search on the packed molecule tables (mnx_substructure_match): for every pair of a query molecule and a
// target molecule whether, how often and where the query embeds in the target. The rule stands in include/molnextr_hip.h
// ("Substructure search"): this library's own, NOT RDKit's HasSubstructMatch and not SMARTS. One launch, one workgroup per pair:
//   the query   admitted as the fingerprint admits a molecule — the atoms' interpretation (atom_symbol.h), the lists and the
//               duplicate test of mol_graph.h — in the arrays the target uses afterwards; what the search needs of it, at most 64
//               atoms, is kept aside: a match word per atom, a 64 x 64 byte matrix of bond words, the order and parent[] (one
//               thread builds them: match_search.h).
//   the target  the same prologue, then every list sorted by neighbour, each by one thread, and a match word per atom written
//               over the dead `info` words.
//   the search  the roots strided over MATCH_LANES lanes; a lane runs match::search depth first on a stack of its own in LDS.
// LDS atomics count degrees and hand out slots of lists that are sorted afterwards, add the embeddings, and take the maximum of
// the steps and the minimum of the roots that have an embedding: a sum, a maximum and a minimum do not depend on the order of
// their operands, so no atomic decides a result and the words are the same from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/molnextr_hip.h"
#include "atom_symbol.h"
#include "atom_write.h"
#include "match_search.h"
#include "mol_graph.h"
#include "table_passes.h"

namespace mnx {

static_assert(sizeof(mnx_match) == 16, "record layout of molnextr_hip.h");
static_assert(MNX_MATCH_MAX_QUERY == match::MAX_QUERY && MNX_MATCH_MAX_QUERY_BONDS == match::MAX_QUERY_BONDS, "one size, one value");
static_assert(match::ANY_BOND == B_ANY + 1u, "the bond word is the class + 1");
static_assert(MNX_MATCH_QUERY_SHIFT == 8 && (MNX_FP_BAD_BOND << MNX_MATCH_QUERY_SHIFT) < MNX_MATCH_LIMIT, "the query's bits below bit 16");

namespace {

constexpr int MATCH_THREADS = MG_THREADS, MATCH_LANES = 128;         // the workgroup; the lanes that search
constexpr unsigned SIDE_REFUSED = PT_TOO_LARGE | PT_BEYOND_TABLES | MNX_FP_BAD_BOND;

// One side's admission, by all threads: mnx_fingerprint_pack's, bit for bit. Leaves info / elem (the atoms' interpretation) and
// off / lst (the lists as the bonds came, the bond word = class + 1) of an admitted molecule; returns bits 0-4. In front: a
// barrier behind the last reader of the arrays. Behind an admitted molecule: graph_duplicate's vote, a barrier.
__device__ __forceinline__ unsigned admit_side(const PackedTables& t, const SymbolTables* __restrict__ st, const Molecule& mol, unsigned* info,
                                               unsigned* elem, unsigned* off, unsigned* cnt, unsigned* lst, unsigned* scan) {
    if (mol.flags & (PT_TOO_LARGE | PT_BEYOND_TABLES)) return mol.flags;
    const unsigned base_flags = mol.flags & PT_TRUNCATED;
    const int na = (int)mol.m.n_atoms;
    int bad = interpret_atoms<MG_MAX, MATCH_THREADS>(t, st, mol, info, elem), pseudo = 0;
    for (int a = threadIdx.x; a < MG_MAX; a += MATCH_THREADS) {       // info[a] is this thread's own entry: no barrier in between
        pseudo |= a < na && info_cls(info[a]) != CLS_ATOM;
        cnt[a] = 0;
    }
    if (__syncthreads_or(bad)) return base_flags | PT_BEYOND_TABLES;
    const unsigned atom_flags = base_flags | (__syncthreads_or(pseudo) ? PT_PSEUDO_ATOM : 0u);
    if (__syncthreads_or(graph_degrees(mol, cnt))) return atom_flags | MNX_FP_BAD_BOND;
    const mnx_bond* B = mol.B;
    graph_lists(mol, cnt, off, scan, lst, [&](int k) { return bond_class(B[k].type) + 1u; });      // `rev` is not read
    if (__syncthreads_or(graph_duplicate(mol, off, lst))) return atom_flags | MNX_FP_BAD_BOND;
    return atom_flags;
}

// an atom's match word (match_search.h) from its interpretation and the two bytes of its element
__device__ __forceinline__ unsigned match_word(unsigned w, unsigned el) {
    const unsigned e0 = el & 255u, e1 = el >> 8 & 255u;
    if (info_cls(w) != CLS_ATOM || (e0 == 'R' && e1 == ' ')) return match::WORD_STAR;       // what put_atom writes as '*'
    return match::atom_word(e0, e1, info_aromatic(w), info_charge(w), info_num(w));
}

__global__ __launch_bounds__(MATCH_THREADS) void match_kernel(
        const PackedTables q, const PackedTables t, const SymbolTables* __restrict__ st, const unsigned* __restrict__ pairs,
        mnx_match* __restrict__ recs, unsigned short* __restrict__ maps, unsigned max_matches, unsigned max_steps) {
    __shared__ unsigned info[MG_MAX], elem[MG_MAX];       // a side's interpretation; then tw = info: the target's match words
    __shared__ unsigned off[MG_MAX + 1], cnt[MG_MAX];
    __shared__ unsigned lst[MG_SLOTS];
    __shared__ unsigned scan[2 * MATCH_THREADS];
    __shared__ unsigned stk[match::MAX_QUERY * MATCH_LANES];          // level k of lane l: stk[k * MATCH_LANES + l], a bank per lane
    __shared__ unsigned char adj[match::MAX_QUERY * match::MAX_QUERY];
    __shared__ unsigned qw[match::MAX_QUERY];
    __shared__ unsigned char order[match::MAX_QUERY], parent[match::MAX_QUERY];
    __shared__ unsigned short img[match::MAX_QUERY];      // the map
    __shared__ unsigned hits, most, win, broken;
    const int p = blockIdx.x, tid = threadIdx.x;
    unsigned short* map = maps + (size_t)p * MNX_MATCH_MAX_QUERY;
    auto refuse = [&](unsigned flags) {
        if (tid < (int)MNX_MATCH_MAX_QUERY) map[tid] = 0xFFFFu;
        if (tid == 0) recs[p] = mnx_match{flags, 0u, 0u, 0u};
    };
    const unsigned qi = pairs[2 * (size_t)p], ti = pairs[2 * (size_t)p + 1];
    if (qi >= (unsigned)q.n || ti >= (unsigned)t.n) { refuse(MNX_MATCH_BAD_PAIR); return; }

    // ---- the query: admitted in the target's arrays, what the search needs of it kept aside ----
    const Molecule qmol = admit_molecule(q, (int)qi);
    unsigned flags = admit_side(q, st, qmol, info, elem, off, cnt, lst, scan) << MNX_MATCH_QUERY_SHIFT;
    const unsigned nq = qmol.m.n_atoms;
    if (!(flags & SIDE_REFUSED << MNX_MATCH_QUERY_SHIFT)) {
        if (nq == 0) flags |= MNX_MATCH_QUERY_EMPTY;
        else if (nq > match::MAX_QUERY || qmol.m.n_bonds > match::MAX_QUERY_BONDS) flags |= MNX_MATCH_QUERY_TOO_LARGE;
    }
    const bool query_ok = !(flags & (SIDE_REFUSED << MNX_MATCH_QUERY_SHIFT | MNX_MATCH_QUERY_EMPTY | MNX_MATCH_QUERY_TOO_LARGE));
    if (query_ok) {
        for (int k = tid; k < (int)sizeof(adj); k += MATCH_THREADS) adj[k] = 0;
        if (tid < (int)nq) qw[tid] = match_word(info[tid], elem[tid]);
        __syncthreads();
        for (int k = tid; k < (int)qmol.m.n_bonds; k += MATCH_THREADS) {       // no pair twice: every byte has one writer
            const unsigned i = qmol.B[k].i, j = qmol.B[k].j;
            adj[i * match::MAX_QUERY + j] = adj[j * match::MAX_QUERY + i] = (unsigned char)(bond_class(qmol.B[k].type) + 1u);
        }
        __syncthreads();
        if (tid == 0) match::build_order(nq, adj, order, parent);
    }
    if (tid == 0) { hits = 0u; most = 0u; win = 0xFFFFFFFFu; broken = 0u; }
    if (tid < (int)match::MAX_QUERY) img[tid] = 0xFFFFu;
    __syncthreads();

    // ---- the target: the prologue of fingerprint_kernel ----
    const Molecule tmol = admit_molecule(t, (int)ti);
    flags |= admit_side(t, st, tmol, info, elem, off, cnt, lst, scan);
    if (!query_ok || (flags & SIDE_REFUSED)) { refuse(flags); return; }
    const int nt = (int)tmol.m.n_atoms;
    unsigned* tw = info;
    for (int a = tid; a < nt; a += MATCH_THREADS) {       // a thread sorts its atoms' lists by neighbour and rewrites its own entries
        const unsigned lo = off[a], hi = off[a + 1];
        for (unsigned u = lo + 1; u < hi; ++u) {
            const unsigned e = lst[u];
            unsigned v = u;
            for (; v > lo && entry_nbr(lst[v - 1]) > entry_nbr(e); --v) lst[v] = lst[v - 1];
            lst[v] = e;
        }
        tw[a] = match_word(info[a], elem[a]);
    }
    __syncthreads();

    // ---- the search: every root by one lane, each to its own end ----
    unsigned* mine = stk + tid;
    if (tid < MATCH_LANES) {
        for (int r = tid; r < nt; r += MATCH_LANES) {
            unsigned found;
            const unsigned steps = match::search((unsigned)r, nq, order, parent, qw, adj, (unsigned)nt, off, lst, tw, mine, (unsigned)MATCH_LANES,
                                                 max_matches, max_steps, &found, [] {});
            if (found) { atomicAdd(&hits, found); atomicMin(&win, (unsigned)r); }
            atomicMax(&most, steps);
            if (steps > max_steps) atomicOr(&broken, 1u);
        }
    }
    __syncthreads();
    // ---- the map: the first embedding of the lowest root that has one, found again by the lane that owns the root ----
    if (win != 0xFFFFFFFFu && tid == (int)(win % MATCH_LANES)) {
        unsigned found;
        match::search(win, nq, order, parent, qw, adj, (unsigned)nt, off, lst, tw, mine, (unsigned)MATCH_LANES, 1u, max_steps, &found, [&] {
            for (unsigned k = 0; k < nq; ++k) img[order[k]] = (unsigned short)match::level_atom(mine[k * MATCH_LANES]);
        });
    }
    __syncthreads();
    if (tid < (int)MNX_MATCH_MAX_QUERY) map[tid] = img[tid];
    if (tid == 0) {
        const unsigned n = min(hits, max_matches);
        recs[p] = mnx_match{flags | (broken && n < max_matches ? MNX_MATCH_LIMIT : 0u), n, most, 0u};
    }
}

}  // namespace

hipError_t match_enqueue(const SymbolTables* st_dev, const PackedTables& q, const PackedTables& t, const unsigned* pairs, int n_pairs,
                         mnx_match* recs, unsigned short* maps, unsigned max_matches, unsigned max_steps, hipStream_t s) {
    hipLaunchKernelGGL(match_kernel, dim3(n_pairs), dim3(MATCH_THREADS), 0, s, q, t, st_dev, pairs, recs, maps, max_matches, max_steps);
    return hipGetLastError();
}

}  // namespace mnx
