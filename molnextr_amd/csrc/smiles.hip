// smiles.hip — a SMILES of the predicted graph from the packed molecule tables of mnx_graph_pack (mnx_smiles_pack): the molecules
// that atom_symbol.h admits and the atoms as it reads them (shared with molfile.hip), the bonds of the bond head, written by a
// depth-first walk after the OpenSMILES grammar. Valid, not canonical (the walk's order is fixed by the atom indices), pseudo-atoms
// as '*'; no stereo (mnx_smiles_pack), or '@' / '@@' at the marked carbons that a wedge begins at (mnx_smiles_pack_stereo: one
// more parallel stage, STEREO, behind the ring numbers), or '/' and '\\' at the double bonds off every cycle (mnx_smiles_pack_marks:
// the stage EZ behind that one). MARKS selects the stages; an instantiation holds none of the code of a stage it does not run.
// mnx_smiles_pack_canonical puts one kernel in front, canon_rank_kernel: canonical atom ranks by partition refinement, one
// workgroup per molecule; count and fill (CANON) then walk by those ranks instead of the atom indices.
// mnx_smiles_pack_symmetric is that call with one more switch, SYM: a candidate of STEREO or EZ with two neighbours of one symmetry
// class on bonds off every cycle writes no mark.
//   count  one workgroup per molecule: the walk and the length of its string -> recs[b].len / flags / n_rings
//   scan   exclusive scan of the lengths over the molecules -> recs[b].text0, totals
//   fill   one workgroup per molecule: the walk again, the bytes behind text0 and the atoms' positions in `order`
// Inside a workgroup: atoms and neighbour lists (mol_graph.h) in parallel, ONE lane for the search and the ring numbers (at most
// 999 atoms and 999 bonds: kept simple), then every atom's piece of the string in parallel, placed by a prefix scan. LDS atomics only
// count degrees and hand out slots of an unsorted list that is sorted afterwards, so no atomic decides a position or an order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/molnextr_hip.h"
#include "atom_symbol.h"
#include "atom_write.h"
#include "block_scan.h"
#include "mol_graph.h"
#include "table_passes.h"

namespace mnx {

static_assert(sizeof(mnx_smiles) == 16, "record layout of molnextr_hip.h");

namespace {

constexpr int SM_THREADS = MG_THREADS, SM_MAX = MG_MAX, SM_PER = MG_PER, SM_SLOTS = MG_SLOTS;     // the sizes of mol_graph.h
constexpr unsigned NONE = 0xFFFFu;
constexpr unsigned REFUSED = PT_TOO_LARGE | PT_BEYOND_TABLES | MNX_SMILES_DUPLICATE_BOND | MNX_SMILES_RING_NUMBERS;

// ---- the writer's own bits of a neighbour-list entry, above neighbour, written class (entry_word) and owner (path_search.h) ----
//   bit 23 a bond of the search tree (to the parent or to a child); every other bond is a ring bond; STEREO only: bit 24 the
//   bond is a wedge (class 5) as the owner sees it, bit 25 a dash (class 6). The rank sorts copy whole entries, so the bits
//   travel with them.
constexpr unsigned SLOT_TREE = 1u << 23, SLOT_UP = 1u << 24, SLOT_DOWN = 1u << 25;
static_assert(SLOT_TREE == 1u << paths::ENTRY_BITS, "the first bit above the shared fields");
__device__ __forceinline__ unsigned slot_seen(unsigned cls) { return cls == 5 ? SLOT_UP : cls == 6 ? SLOT_DOWN : 0u; }
__device__ __forceinline__ long long slot_z(unsigned e) { return (long long)(e >> 24 & 1u) - (long long)(e >> 25 & 1u); }

// det of the rows a, b, c, exact in 64 bits (|x|, |y| < 2^18 and |z| <= 2 here)
__device__ __forceinline__ long long det3(long long ax, long long ay, long long az, long long bx, long long by, long long bz,
                                          long long cx, long long cy, long long cz) {
    return ax * (by * cz - bz * cy) - ay * (bx * cz - bz * cx) + az * (bx * cy - by * cx);
}

// the byte of a bond between two atoms, 0 = written as nothing
__device__ __forceinline__ char bond_symbol(unsigned cls, bool both_aromatic) {
    switch (cls) {
        case B_SINGLE: return both_aromatic ? '-' : 0;
        case B_DOUBLE: return '=';
        case B_TRIPLE: return '#';
        case B_AROMATIC: return both_aromatic ? 0 : ':';
        default: return '~';
    }
}

// ---- EZ: what the atoms carry between its stages, in arrays of the search that are dead by then ----
//   role (done_last)       ROLE_B: the bond to the parent is a resolved candidate (this atom is its b), ROLE_A: this atom is the a
//                          of one, with its flip before forcing in bit 2; ROLE_UNRESOLVED: b of a candidate that got no marks
//   child_dir (done_child) bit 0: the bond parent -> this atom takes a symbol from the candidate the parent is an end of, bit 1:
//                          this atom lies on the left of that candidate's axis; in the end the symbol itself, 0 for none
//   low, then flip (cur)   the lowest written position a ring bond reaches from the atom's subtree; then a's flip
//   SYM adds ROLE_SYM at both ends of a candidate dropped for symmetry, and bit 2 of an atom's mark in stk (MNX_ATOM_MARK_SYM)
constexpr unsigned ROLE_B = 1, ROLE_A = 2, ROLE_F0 = 4, ROLE_UNRESOLVED = 8, ROLE_SYM = 16;

// ---- canonical ranks (mnx_smiles_pack_canonical; the rule: molnextr_hip.h) ----
constexpr unsigned CANON_BITS = MNX_SMILES_CANON_TIE | MNX_SMILES_CANON_TIE_INDEX;
static_assert(SM_THREADS == 4 * 64, "block_min: four waves of 64");

// the smallest of one value per thread, to every thread; red holds four values. Ends with a barrier.
__device__ __forceinline__ unsigned long long block_min(unsigned long long v, unsigned long long* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const unsigned long long a = red[0] < red[1] ? red[0] : red[1], c = red[2] < red[3] ? red[2] : red[3];
    __syncthreads();
    return a < c ? a : c;
}

// One workgroup per molecule: rank[atom0 + a] and sym_class[atom0 + a] (may be null) of every atom, 0xFFFF where the molecule
// is refused on flag bits 0, 1 or 4, and the tie bits in recs[b].flags (0 without one), which count keeps. The prologue:
// admission and the atoms' interpretation (atom_symbol.h), the unsorted lists and the duplicate test of mol_graph.h. The
// keys never leave LDS: per round every list entry becomes r(n) * 8 + c (13 bits), each list is rank-sorted, and an atom's
// new rank is a count over the other atoms, its list compared only with those of equal old rank (which have its degree: the
// first key holds it and a round only splits classes). No atomic decides a rank: the lists are sorted by value each round.
__global__ __launch_bounds__(SM_THREADS) void canon_rank_kernel(
        const PackedTables t, const SymbolTables* __restrict__ st, mnx_smiles* __restrict__ recs,
        unsigned short* __restrict__ rank, unsigned short* __restrict__ sym_class) {
    __shared__ unsigned info[SM_MAX], elem[SM_MAX];
    __shared__ unsigned off[SM_MAX + 1], cnt[SM_MAX];
    __shared__ unsigned raw[SM_SLOTS];                    // the lists as the bonds came: neighbour, class, owner
    __shared__ unsigned short key[SM_SLOTS], lst[SM_SLOTS];   // a round's entries r(n) * 8 + c as the lists stand, then sorted
    __shared__ unsigned long long text8[SM_MAX];          // an atom's written bytes 0-7 (the first in the top byte) and 8-11,
    __shared__ unsigned text4[SM_MAX];                    // zeros behind the last: a prefix compares smaller
    __shared__ unsigned xy[SM_MAX];                       // x_bin << 16 | y_bin
    __shared__ unsigned short rk[SM_MAX];
    __shared__ unsigned scan[2 * SM_THREADS];
    __shared__ unsigned long long red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const Molecule mol = admit_molecule(t, b);
    const mnx_mol& m = mol.m;
    auto refuse = [&]() {
        for (unsigned a = tid; a < m.n_atoms && (unsigned long long)m.atom0 + a < t.n_atom_records; a += SM_THREADS) {
            rank[m.atom0 + a] = (unsigned short)NONE;
            if (sym_class) sym_class[m.atom0 + a] = (unsigned short)NONE;
        }
        if (tid == 0) recs[b].flags = 0;
    };
    if (mol.flags & (PT_TOO_LARGE | PT_BEYOND_TABLES)) { refuse(); return; }
    const int na = (int)m.n_atoms, nb = (int)m.n_bonds;
    const mnx_bond* B = mol.B;

    int bad = interpret_atoms<SM_MAX, SM_THREADS>(t, st, mol, info, elem);
    for (int a = tid; a < SM_MAX; a += SM_THREADS) {
        cnt[a] = 0;
        xy[a] = a < na ? (unsigned)mol.A[a].x_bin << 16 | mol.A[a].y_bin : 0u;
    }
    __syncthreads();
    bad |= graph_degrees(mol, cnt);
    if (__syncthreads_or(bad)) { refuse(); return; }
    graph_lists(mol, cnt, off, scan, raw, [&](int k) { return bond_class(B[k].type); });      // any slot: every round sorts by value
    if (__syncthreads_or(graph_duplicate(mol, off, raw))) { refuse(); return; }

    // ---- the initial key: the atom's written bytes (12 at most: '[', three digits, two letters, 'H' digit, sign and two
    //      digits, ']'), then its degree ----
    for (int a = tid; a < na; a += SM_THREADS) {
        unsigned long long hi = 0;
        unsigned lo = 0, n = 0;
        put_atom(info[a], elem[a], 0u, [&](char c) {
            if (n < 8u) hi |= (unsigned long long)(unsigned char)c << (56u - 8u * n);
            else if (n < 12u) lo |= (unsigned)(unsigned char)c << (24u - 8u * (n - 8u));
            ++n;
        });
        text8[a] = hi;
        text4[a] = lo;
    }
    __syncthreads();
    for (int a = tid; a < na; a += SM_THREADS) {
        const unsigned long long hi = text8[a];
        const unsigned lo = text4[a], deg = off[a + 1] - off[a];
        unsigned less = 0;
        for (int o = 0; o < na; ++o) {
            const unsigned long long h = text8[o];
            const unsigned l = text4[o], d = off[o + 1] - off[o];
            less += h < hi || (h == hi && (l < lo || (l == lo && d < deg)));
        }
        rk[a] = (unsigned short)less;
    }
    __syncthreads();

    // ---- one refinement round over the ranks in rk: whether a rank changed (a round that splits no class changes none), and
    //      in vmin the lowest new rank among this thread's atoms that another atom shares ----
    unsigned vmin = NONE;
    auto round = [&]() {
        for (int s = tid; s < 2 * nb; s += SM_THREADS) key[s] = (unsigned short)(rk[entry_nbr(raw[s])] * 8u + entry_word(raw[s]));
        __syncthreads();
        for (int s = tid; s < 2 * nb; s += SM_THREADS) {
            const unsigned a = entry_owner(raw[s]), mine = key[s];
            unsigned at = off[a];
            for (unsigned u = off[a]; u < off[a + 1]; ++u) at += key[u] < mine || (key[u] == mine && u < (unsigned)s);
            lst[at] = (unsigned short)mine;
        }
        __syncthreads();
        unsigned r[SM_PER], less[SM_PER], same[SM_PER];
#pragma unroll
        for (int q = 0; q < SM_PER; ++q) {
            const int a = tid + q * SM_THREADS;
            r[q] = a < na ? rk[a] : NONE;                 // NONE: no atom, nothing below is kept
            less[q] = same[q] = 0;
        }
        for (int o = 0; o < na; ++o) {
            const unsigned ro = rk[o];
#pragma unroll
            for (int q = 0; q < SM_PER; ++q) {
                const int a = tid + q * SM_THREADS;
                if (ro < r[q]) ++less[q];
                else if (ro == r[q] && o != a) {
                    const unsigned la = off[a], lo = off[o], d = off[a + 1] - la;
                    int c = 0;
                    for (unsigned k = 0; k < d && c == 0; ++k) c = (int)lst[lo + k] - (int)lst[la + k];
                    less[q] += c < 0;
                    same[q] += c == 0;
                }
            }
        }
        int changed = 0;
        vmin = NONE;
#pragma unroll
        for (int q = 0; q < SM_PER; ++q) {
            if (tid + q * SM_THREADS >= na) continue;
            changed |= less[q] != r[q];
            if (same[q]) vmin = min(vmin, less[q]);
        }
        changed = __syncthreads_or(changed);              // every thread has read the old ranks
#pragma unroll
        for (int q = 0; q < SM_PER; ++q)
            if (tid + q * SM_THREADS < na) rk[tid + q * SM_THREADS] = (unsigned short)less[q];
        __syncthreads();
        return changed;
    };

    // ---- refine, break the lowest tie, refine again. The number of distinct ranks rises in every round but the last of a pass
    //      and at every tie, from 1 at least to n_atoms: at most n_atoms passes, and in each at most n_atoms rounds (over all
    //      passes at most 2 * n_atoms rounds). A round costs a thread at most 4 * n_atoms list comparisons. ----
    unsigned flags = 0;
    for (int pass = 0; pass < na; ++pass) {
        for (int k = 0; k < na; ++k)
            if (!round()) break;
        if (pass == 0 && sym_class)
            for (int a = tid; a < na; a += SM_THREADS) sym_class[m.atom0 + a] = rk[a];
        const unsigned long long v = block_min(vmin, red);
        if (v == NONE) break;                             // no rank is shared: a permutation
        unsigned long long best = ~0ull;
        for (int a = tid; a < na; a += SM_THREADS)
            if (rk[a] == v) best = min(best, (unsigned long long)xy[a] << 16 | (unsigned)a);
        best = block_min(best, red);                      // the smallest (x_bin, y_bin, atom index) keeps v
        int by_index = 0;
        for (int a = tid; a < na; a += SM_THREADS)
            if (rk[a] == v && (unsigned)a != (unsigned)(best & 0xFFFFu)) {
                by_index |= xy[a] == (unsigned)(best >> 16);
                rk[a] = (unsigned short)(v + 1u);
            }
        by_index = __syncthreads_or(by_index);
        flags |= MNX_SMILES_CANON_TIE | (by_index ? MNX_SMILES_CANON_TIE_INDEX : 0u);
    }
    for (int a = tid; a < na; a += SM_THREADS) rank[m.atom0 + a] = rk[a];
    if (tid == 0) recs[b].flags = flags;
}

// CANON (mnx_smiles_pack_canonical): the walk runs on the ranks that canon_rank_kernel left in `rank` instead of on the atom
// indices — the first sort of the lists and the order of the roots; every later stage works on written positions as it is.
// SYM (mnx_smiles_pack_symmetric, CANON only): a candidate of either stage with an equal pair (two neighbours of one class in
// `sym_class`, read from global: a handful of reads per candidate, so the classes take no LDS; both on bonds off every cycle)
// writes no mark. The low[] pass of EZ then runs in front of STEREO, for every set of marks but 0. fill leaves every atom's
// MNX_ATOM_* bits in `atom_marks` (may be null), one owner thread per byte.
template <bool FILL, unsigned MARKS, bool CANON = false, bool SYM = false>
__global__ __launch_bounds__(SM_THREADS) void smiles_kernel(
        const PackedTables t, const SymbolTables* __restrict__ st, mnx_smiles* __restrict__ recs,
        unsigned short* __restrict__ order, char* __restrict__ out, unsigned out_cap, const unsigned short* __restrict__ rank,
        const unsigned short* __restrict__ sym_class, unsigned char* __restrict__ atom_marks) {
    static_assert(CANON || !SYM, "the symmetry rule reads the classes of the rank kernel");
    __shared__ unsigned short rnk[CANON ? SM_MAX : 1], inv[CANON ? SM_MAX : 1];     // atom -> rank, rank -> atom
    __shared__ unsigned info[SM_MAX], elem[SM_MAX];
    __shared__ unsigned off[SM_MAX + 1], cnt[SM_MAX];     // an atom's list is [off[a], off[a + 1]); cnt: degrees, then fill cursors
    __shared__ unsigned raw[SM_SLOTS], adj[SM_SLOTS];     // the lists as the bonds came, then in ascending neighbour index
    __shared__ unsigned scan[2 * SM_THREADS];
    __shared__ unsigned short pos[SM_MAX], at[SM_MAX];    // atom -> written position, position -> atom
    __shared__ unsigned short parent[SM_MAX], stk[SM_MAX], cur[SM_MAX];   // stk: the search's stack, then (STEREO) every atom's mark
    __shared__ unsigned short done_child[SM_MAX], done_last[SM_MAX];  // the child an atom returned from, the atom written last inside it
                                                          // (EZ: cur, done_child and done_last carry its state behind the search)
    __shared__ unsigned short closes[SM_MAX];             // ')' behind an atom's text
    __shared__ unsigned char paren[SM_MAX], rnum[SM_SLOTS];
    __shared__ unsigned walk[2];                          // components, 1 = more than 99 ring numbers in use
    constexpr bool STEREO = (MARKS & MNX_SMILES_MARK_TETRAHEDRAL) != 0, EZ = (MARKS & MNX_SMILES_MARK_DOUBLE_BOND) != 0;
    const int b = blockIdx.x, tid = threadIdx.x;
    const Molecule mol = admit_molecule(t, b);
    const mnx_mol& m = mol.m;
    const unsigned base_flags = mol.flags & PT_TRUNCATED;
    auto record = [&](unsigned len, unsigned flags, unsigned n_rings) {     // count's result; len 0 with a bit of REFUSED = refused
        if (tid == 0) {                                   // CANON: the rank kernel left the tie bits there
            if (CANON) flags |= recs[b].flags & CANON_BITS;
            recs[b].len = len; recs[b].flags = flags; recs[b].n_rings = n_rings;
        }
    };
    unsigned text0 = 0;
    bool sym_on = SYM;                                    // SYM: the rule is off for a molecule that holds a pseudo-atom
    if (FILL) {
        const mnx_smiles r = recs[b];
        if (r.len == 0) {                                 // no string (the same for every thread): its atoms get no position
            if ((order || (SYM && atom_marks)) && (r.flags & REFUSED))
                for (unsigned a = tid; a < m.n_atoms && (unsigned long long)m.atom0 + a < t.n_atom_records; a += SM_THREADS) {
                    if (order) order[m.atom0 + a] = (unsigned short)NONE;
                    if (SYM && atom_marks) atom_marks[m.atom0 + a] = 0xFFu;
                }
            return;
        }
        text0 = r.text0;
        if (SYM) sym_on = !(r.flags & PT_PSEUDO_ATOM);
    } else if (mol.flags & (PT_TOO_LARGE | PT_BEYOND_TABLES)) {
        record(0, mol.flags, 0);
        return;
    }
    const int na = (int)m.n_atoms, nb = (int)m.n_bonds;
    const mnx_bond* B = mol.B;
    // a record's `type`; CANON: of the record renumbered by the ranks, which has the lower rank as i — where the ends swap,
    // `type` and `rev` swap (what each end sees of the bond, SLOT_UP / SLOT_DOWN below, stays with the end)
    auto type_of = [&](int k, unsigned i, unsigned j) -> unsigned { return CANON && rnk[i] > rnk[j] ? B[k].rev : B[k].type; };

    // ---- every atom's interpretation and the walk's own per-atom state, every bond's degree counts; a record that points
    //      beyond its table refuses the molecule ----
    int bad = interpret_atoms<SM_MAX, SM_THREADS>(t, st, mol, info, elem), pseudo = 0, wedge = 0, any = 0;
    for (int a = tid; a < SM_MAX; a += SM_THREADS) {      // info[a] is this thread's own entry: no barrier in between
        pseudo |= a < na && info_cls(info[a]) != CLS_ATOM;
        cnt[a] = 0;
        pos[a] = (unsigned short)NONE;
        closes[a] = 0;
        paren[a] = 0;
        if (CANON) rnk[a] = a < na ? rank[m.atom0 + a] : (unsigned short)NONE;
    }
    __syncthreads();
    bad |= graph_degrees(mol, cnt, [&](int k, unsigned i, unsigned j) {     // (a record with i == j: the molfile writer writes it)
        const unsigned ty = type_of(k, i, j);
        wedge |= ty == 5 || ty == 6;
        any |= ty < 1 || ty > 6;
    });
    if (__syncthreads_or(bad)) {                          // (count refuses; fill never comes here: count left len = 0)
        if (!FILL) record(0, base_flags | PT_BEYOND_TABLES, 0);
        return;
    }
    if (!FILL) {
        pseudo = __syncthreads_or(pseudo);
        wedge = __syncthreads_or(wedge);
        any = __syncthreads_or(any);
        if (SYM) sym_on = !pseudo;
    }

    // ---- neighbour lists: entries as the bonds come (end 0 sees edges[i][j], end 1 edges[j][i]), then each list in ascending order ----
    graph_lists(mol, cnt, off, scan, raw, [&](int k) { return bond_class(type_of(k, B[k].i, B[k].j)); },
                [&](int k, int end) { return STEREO ? slot_seen(end ? B[k].rev : B[k].type) : 0u; });
    int dup = 0;
    for (int s = tid; s < 2 * nb; s += SM_THREADS) {      // rank of every entry inside its list, with mol_graph.h's duplicate test
        const unsigned e = raw[s], mine = entry_nbr(e), a = entry_owner(e);
        unsigned rank = 0;
        for (unsigned t = off[a]; t < off[a + 1]; ++t) {
            const unsigned n = entry_nbr(raw[t]);
            if (CANON) rank += rnk[n] < rnk[mine] || (rnk[n] == rnk[mine] && t < (unsigned)s);
            else rank += n < mine || (n == mine && t < (unsigned)s);
            dup |= graph_twice(n, t, mine, (unsigned)s);
        }
        adj[off[a] + rank] = e;
    }
    dup = __syncthreads_or(dup);
    if (CANON) {                                          // a duplicate pair left no ranks (0xFFFF): the search below, which
        for (int a = tid; a < SM_MAX; a += SM_THREADS) {  // then only counts the components, runs on the indices
            if (dup) rnk[a] = (unsigned short)a;
            inv[a] = (unsigned short)a;
        }
        __syncthreads();
        for (int a = tid; a < na; a += SM_THREADS)
            if (rnk[a] < SM_MAX) inv[rnk[a]] = (unsigned short)a;
        __syncthreads();
    }

    // ---- the search, by one lane: depth-first from the lowest atom of every component, neighbours in ascending index, an
    //      explicit stack (a path of 999 atoms is 998 deep). It leaves the written order, the tree bonds, the parentheses. ----
    if (tid == 0) {
        unsigned written = 0, comps = 0;
        for (int k = 0; k < na; ++k) {
            const int root = CANON ? (int)inv[k] : k;
            if (pos[root] != NONE) continue;
            ++comps;
            int sp = 0;
            stk[0] = (unsigned short)root;
            parent[root] = (unsigned short)NONE;
            done_child[root] = (unsigned short)NONE;
            cur[root] = (unsigned short)off[root];
            pos[root] = (unsigned short)written;
            at[written++] = (unsigned short)root;
            while (sp >= 0) {
                const unsigned a = stk[sp], c = cur[a];
                if (c == off[a + 1]) {                    // a is finished: its parent remembers it and the atom written last
                    if (--sp >= 0) {
                        const unsigned p = stk[sp];
                        done_child[p] = (unsigned short)a;
                        done_last[p] = at[written - 1];
                    }
                    continue;
                }
                cur[a] = (unsigned short)(c + 1);
                const unsigned n = entry_nbr(adj[c]);
                if (n == parent[a]) { adj[c] |= SLOT_TREE; continue; }
                if (pos[n] != NONE) continue;             // a ring bond
                adj[c] |= SLOT_TREE;
                if (done_child[a] != NONE) {              // a further child: the one before it goes inside parentheses
                    paren[done_child[a]] = 1;
                    closes[done_last[a]] += 1;
                }
                parent[n] = (unsigned short)a;
                done_child[n] = (unsigned short)NONE;
                cur[n] = (unsigned short)off[n];
                pos[n] = (unsigned short)written;
                at[written++] = (unsigned short)n;
                stk[++sp] = (unsigned short)n;
            }
        }
        walk[0] = comps;
        walk[1] = 0;
    }
    __syncthreads();
    const unsigned n_rings = (unsigned)nb + walk[0] - (unsigned)na;
    if (dup) {                                            // (count refuses; fill never comes here)
        if (!FILL) record(0, base_flags | (pseudo ? PT_PSEUDO_ATOM : 0u) | MNX_SMILES_DUPLICATE_BOND, n_rings);
        return;
    }

    // ---- every list once more, now in ascending written position of the neighbour: ring closures, then ring openings ----
    for (int s = tid; s < 2 * nb; s += SM_THREADS) {
        const unsigned e = adj[s], mine = pos[entry_nbr(e)], a = entry_owner(e);
        unsigned rank = 0;
        for (unsigned t = off[a]; t < off[a + 1]; ++t) rank += pos[entry_nbr(adj[t])] < mine;
        raw[off[a] + rank] = e;
    }
    __syncthreads();

    // ---- ring numbers, by the same lane, atoms in written order: a free mask of 99 bits; what an atom closes is free from
    //      the next atom on. An opening writes its number into the entries of both ends. ----
    if (tid == 0) {
        unsigned long long used[2] = {0, 0}, closed[2] = {0, 0};
        unsigned in_use = 0, fail = 0;
        for (int p = 0; p < na; ++p) {
            const unsigned a = at[p];
            in_use -= (unsigned)(__popcll(closed[0]) + __popcll(closed[1]));
            used[0] &= ~closed[0]; used[1] &= ~closed[1];
            closed[0] = closed[1] = 0;
            unsigned opens = 0;
            for (unsigned s = off[a]; s < off[a + 1]; ++s) opens += !(raw[s] & SLOT_TREE) && pos[entry_nbr(raw[s])] > (unsigned)p;
            if (in_use + opens > 99u) { fail = 1; break; }
            for (unsigned s = off[a]; s < off[a + 1]; ++s) {
                const unsigned e = raw[s], n = entry_nbr(e);
                if (e & SLOT_TREE) continue;
                if (pos[n] < (unsigned)p) {
                    const unsigned k = rnum[s] - 1u;
                    closed[k >> 6] |= 1ull << (k & 63u);
                    continue;
                }
                const unsigned k = ~used[0] ? (unsigned)__ffsll((long long)~used[0]) - 1u : 64u + (unsigned)__ffsll((long long)~used[1]) - 1u;
                used[k >> 6] |= 1ull << (k & 63u);
                ++in_use;
                rnum[s] = (unsigned char)(k + 1u);
                unsigned lo = off[n], hi = off[n + 1] - 1u;           // n's entry for a: its list is ordered by written position
                while (lo < hi) {
                    const unsigned mid = (lo + hi) >> 1;
                    if (pos[entry_nbr(raw[mid])] < (unsigned)p) lo = mid + 1u; else hi = mid;
                }
                rnum[lo] = (unsigned char)(k + 1u);
            }
        }
        walk[1] = fail;
    }
    __syncthreads();
    if (walk[1]) {                                        // (count refuses; fill never comes here)
        if (!FILL) record(0, base_flags | (pseudo ? PT_PSEUDO_ATOM : 0u) | MNX_SMILES_RING_NUMBERS, n_rings);
        return;
    }

    // ---- SYM: the lowest written position a ring bond reaches from every atom's subtree, in front of both stages (EZ's own
    //      pass, which `cur` holds until EZ turns it into the flips). A tree bond parent -> x is off every cycle iff
    //      low[x] >= pos[x]; a ring bond never is. ----
    if (SYM && MARKS != 0u) {
        for (int a = tid; a < na; a += SM_THREADS) {
            unsigned l = NONE;
            for (unsigned s = off[a]; s < off[a + 1]; ++s)
                if (!(raw[s] & SLOT_TREE)) l = min(l, (unsigned)pos[entry_nbr(raw[s])]);
            cur[a] = (unsigned short)l;
        }
        __syncthreads();
        if (tid == 0)
            for (int p = na - 1; p > 0; --p) {
                const unsigned a = at[p], par = parent[a];
                if (par != NONE && cur[a] < cur[par]) cur[par] = cur[a];
            }
        __syncthreads();
    }
    // an equal pair at u: two neighbours other than `skip` of one class, both on bonds off every cycle
    auto equal_pair = [&](unsigned u, unsigned skip) {
        auto free_nbr = [&](unsigned e) {                 // the neighbour of a list entry of u, NONE where the bond is on a cycle
            const unsigned n = entry_nbr(e), x = pos[n] < pos[u] ? u : n;
            return (e & SLOT_TREE) && n != skip && cur[x] >= pos[x] ? n : NONE;
        };
        for (unsigned s = off[u]; s + 1 < off[u + 1]; ++s) {
            const unsigned n1 = free_nbr(raw[s]);
            if (n1 == NONE) continue;
            const unsigned c1 = sym_class[m.atom0 + n1];
            for (unsigned q = s + 1; q < off[u + 1]; ++q) {
                const unsigned n2 = free_nbr(raw[q]);
                if (n2 != NONE && sym_class[m.atom0 + n2] == c1) return true;
            }
        }
        return false;
    };
    auto mark_of = [&](unsigned a) -> unsigned { return SYM ? stk[a] & 3u : stk[a]; };

    // ---- STEREO: every marked carbon that a wedge begins at, in parallel over the atoms (the rule: molnextr_hip.h). An atom's
    //      list stands in ascending written position, so the string's neighbour order is: the parent (group 0), the ring items
    //      in list order (group 1), the children in list order (group 2). The determinant is taken over the list as it stands
    //      and flips with the parity of the permutation into that order: it is alternating in the neighbours. ----
    int marked = 0, unresolved = 0, dropped = 0, sym_dropped = 0;
    if (STEREO) {
        for (int a = tid; a < na; a += SM_THREADS) {
            const unsigned w = info[a], lo = off[a], hi = off[a + 1], p = pos[a];
            unsigned mark = 0, sym = 0;
            if (w & 8u) {
                unsigned seen = 0, other = 0;
                for (unsigned s = lo; s < hi; ++s) {
                    seen |= raw[s] & (SLOT_UP | SLOT_DOWN);
                    other |= entry_word(raw[s]) != B_SINGLE;
                }
                const unsigned deg = hi - lo;
                const bool candidate = seen && !other && info_cls(w) == CLS_ATOM && deg + (unsigned)info_h(w) == 4u;
                if (SYM && sym_on && candidate) sym = equal_pair((unsigned)a, NONE);      // symmetry first: no determinant then
                if (candidate && !sym) {
                    const unsigned e0 = raw[lo], e1 = raw[lo + 1], e2 = raw[lo + 2], e3 = deg == 4u ? raw[lo + 3] : e2;
                    auto group = [&](unsigned e) { return !(e & SLOT_TREE) ? 1 : pos[entry_nbr(e)] < p ? 0 : 2; };
                    const long long cx = mol.A[a].x_bin, cy = mol.A[a].y_bin;
                    const mnx_atom A0 = mol.A[entry_nbr(e0)], A1 = mol.A[entry_nbr(e1)], A2 = mol.A[entry_nbr(e2)], A3 = mol.A[entry_nbr(e3)];
                    const long long x0 = A0.x_bin - cx, y0 = cy - A0.y_bin, z0 = slot_z(e0);      // the image's y points down
                    const long long x1 = A1.x_bin - cx, y1 = cy - A1.y_bin, z1 = slot_z(e1);
                    const long long x2 = A2.x_bin - cx, y2 = cy - A2.y_bin, z2 = slot_z(e2);
                    const long long x3 = A3.x_bin - cx, y3 = cy - A3.y_bin, z3 = slot_z(e3);
                    const int g0 = group(e0), g1 = group(e1), g2 = group(e2), g3 = group(e3);
                    int flips = (g0 > g1) + (g0 > g2) + (g1 > g2);
                    long long d;
                    if (deg == 4u) {
                        flips += (g0 > g3) + (g1 > g3) + (g2 > g3);
                        d = det3(x1 - x0, y1 - y0, z1 - z0, x2 - x0, y2 - y0, z2 - z0, x3 - x0, y3 - y0, z3 - z0);
                    } else {
                        flips += parent[a] != NONE;       // the implicit H stands behind a parent: an odd position of the four
                        d = det3(x0, y0, z0, x1, y1, z1, x2, y2, z2);
                    }
                    if (flips & 1) d = -d;
                    mark = d < 0 ? 1u : d > 0 ? 2u : 0u;
                }
                unresolved |= seen && !mark && !sym;
            }
            marked |= mark != 0;
            sym_dropped |= (int)sym;
            stk[a] = (unsigned short)(mark | sym << 2);
        }
        if (FILL) __syncthreads();
        else {
            marked = __syncthreads_or(marked);
            unresolved = __syncthreads_or(unresolved);
            for (int k = tid; k < nb; k += SM_THREADS) {  // a wedge neither end of which received a mark
                const unsigned ty = type_of(k, B[k].i, B[k].j);
                dropped |= (ty == 5 || ty == 6) && !mark_of(B[k].i) && !mark_of(B[k].j);
            }
            dropped = __syncthreads_or(dropped);
        }
    }

    // ---- EZ: '/' and '\' at every candidate double bond that resolves (the rule: molnextr_hip.h). A candidate lies on no cycle,
    //      so it is the tree bond into its later-written end b, and no ring bond joins b's subtree to an atom written before b.
    //      Each atom belongs to at most one candidate (its other bonds are single), so the thread of b owns the whole candidate
    //      and is the only writer of what it leaves at a, at b and at their children. ----
    int directed = 0, ez_unresolved = 0, implied = 0;
    if (EZ) {
        unsigned short *low = cur, *flip = cur, *child_dir = done_child, *role = done_last;
        const mnx_atom* A = mol.A;
        for (int a = tid; a < na; a += SM_THREADS) {
            if (!SYM) {                                   // (SYM: low stands since the pass in front of STEREO)
                unsigned l = NONE;
                for (unsigned s = off[a]; s < off[a + 1]; ++s)
                    if (!(raw[s] & SLOT_TREE)) l = min(l, (unsigned)pos[entry_nbr(raw[s])]);
                low[a] = (unsigned short)l;
            }
            child_dir[a] = 0;
            role[a] = 0;
        }
        __syncthreads();
        if (!SYM) {
            if (tid == 0)                                 // minimised up the tree: children are written behind their parent
                for (int p = na - 1; p > 0; --p) {
                    const unsigned a = at[p], par = parent[a];
                    if (par != NONE && low[a] < low[par]) low[par] = low[a];
                }
            __syncthreads();
        }
        for (int c = tid; c < na; c += SM_THREADS) {
            const unsigned a = parent[c];
            if (a == NONE || low[c] < pos[c]) continue;
            if (info_cls(info[c]) != CLS_ATOM || info_cls(info[a]) != CLS_ATOM) continue;
            const unsigned dc = off[c + 1] - off[c], da = off[a + 1] - off[a];
            if (dc < 2u || dc > 3u || da < 2u || da > 3u) continue;
            const long long ax = (long long)A[c].x_bin - (long long)A[a].x_bin, ay = (long long)A[a].y_bin - (long long)A[c].y_bin;
            auto side = [&](unsigned u, unsigned n) {         // the image's y points down
                const long long vx = (long long)A[n].x_bin - (long long)A[u].x_bin, vy = (long long)A[u].y_bin - (long long)A[n].y_bin;
                const long long d = ax * vy - ay * vx;
                return d > 0 ? 1 : d < 0 ? -1 : 0;
            };
            bool candidate = true, resolved = true;
            for (int end = 0; end < 2; ++end) {
                const unsigned u = end ? (unsigned)c : a, v = end ? a : (unsigned)c;
                int before = 0;
                for (unsigned s = off[u]; s < off[u + 1]; ++s) {
                    const unsigned e = raw[s], n = entry_nbr(e);
                    if (n == v) { candidate &= entry_word(e) == B_DOUBLE; continue; }
                    candidate &= entry_word(e) == B_SINGLE;
                    const int sd = side(u, n);
                    resolved &= sd != 0 && sd != before;
                    before = sd;
                }
            }
            if (!candidate) continue;
            if (SYM && sym_on && (equal_pair(a, (unsigned)c) || equal_pair((unsigned)c, a))) {    // no symbols, no part in the flips
                role[c] = role[a] = (unsigned short)ROLE_SYM;
                continue;
            }
            if (!resolved) { role[c] = (unsigned short)ROLE_UNRESOLVED; continue; }
            unsigned f0 = 2;                              // the flip that makes the first directed bond of the list '/'
            for (int end = 0; end < 2; ++end) {
                const unsigned u = end ? (unsigned)c : a, v = end ? a : (unsigned)c;
                for (unsigned s = off[u]; s < off[u + 1]; ++s) {        // tree bonds in written order: a's parent, then the children
                    const unsigned e = raw[s], n = entry_nbr(e);
                    if (n == v || !(e & SLOT_TREE)) continue;
                    const unsigned up = side(u, n) > 0;
                    if (pos[n] < pos[u]) f0 = up;
                    else {
                        child_dir[n] = (unsigned short)(1u | up << 1);
                        if (f0 == 2u) f0 = !up;
                    }
                }
            }
            role[c] = (unsigned short)ROLE_B;
            role[a] = (unsigned short)(ROLE_A | (f0 & 1u) * ROLE_F0);
        }
        __syncthreads();
        if (tid == 0)                                     // a's flip, in written order: forced when an earlier candidate gave the
            for (int p = 0; p < na; ++p) {                // bond to a's parent its symbol
                const unsigned a = at[p], r = role[a];
                if (!(r & ROLE_A)) continue;
                unsigned f = (r & ROLE_F0) != 0;
                const unsigned d = child_dir[a];
                if (d & 1u) {
                    const unsigned par = parent[a], first = role[par] & ROLE_A ? par : parent[par];
                    f ^= 1u ^ (d >> 1 & 1u) ^ flip[first];
                }
                flip[a] = (unsigned short)f;
            }
        __syncthreads();
        for (int x = tid; x < na; x += SM_THREADS) {      // the symbol in front of x
            const unsigned d = child_dir[x], r = role[x];
            unsigned sym = 0;
            if (d & 1u) {
                const unsigned par = parent[x], first = role[par] & ROLE_A ? par : parent[par];
                sym = (d >> 1 & 1u) ^ flip[first] ? '/' : '\\';
            } else if ((r & ROLE_A) && parent[x] != NONE) sym = '/';
            child_dir[x] = (unsigned short)sym;
            directed |= sym != 0;
            ez_unresolved |= (r & ROLE_UNRESOLVED) != 0;
            if (SYM) sym_dropped |= (r & ROLE_SYM) != 0;
        }
        if (FILL) __syncthreads();
        else {
            directed = __syncthreads_or(directed);
            ez_unresolved = __syncthreads_or(ez_unresolved);
            auto has_directed = [&](unsigned u) {
                unsigned any_dir = child_dir[u];
                for (unsigned s = off[u]; s < off[u + 1]; ++s)
                    if ((raw[s] & SLOT_TREE) && pos[entry_nbr(raw[s])] > pos[u]) any_dir |= child_dir[entry_nbr(raw[s])];
                return any_dir != 0;
            };
            for (int k = tid; k < nb; k += SM_THREADS) {  // a double bond without marks of its own between two directed bonds
                const unsigned i = B[k].i, j = B[k].j;
                if (type_of(k, i, j) != 2) continue;
                constexpr unsigned OWN = ROLE_B | (SYM ? ROLE_SYM : 0u);   // (a double bond into an end of a symmetric candidate is it)
                const bool mine = (parent[j] == i && (role[j] & OWN)) || (parent[i] == j && (role[i] & OWN));
                implied |= !mine && has_directed(i) && has_directed(j);
            }
            implied = __syncthreads_or(implied);
        }
    }

    // ---- the piece of the atom at written position p: '.' or '(' and the bond from its parent, its text, its ring items, the
    //      ')' of every branch that ends behind it ----
    auto piece = [&](unsigned p, auto put) {
        const unsigned a = at[p], w = info[a], par = parent[a];
        const bool aromatic = info_aromatic(w);
        if (par == NONE) {
            if (p > 0) put('.');
        } else {
            if (paren[a]) put('(');
            for (unsigned s = off[a]; s < off[a + 1]; ++s) {
                const unsigned e = raw[s];
                if ((e & SLOT_TREE) && entry_nbr(e) == par) {
                    const char c = EZ && done_child[a] ? (char)done_child[a] : bond_symbol(entry_word(e), aromatic && info_aromatic(info[par]));
                    if (c) put(c);
                    break;
                }
            }
        }
        put_atom(w, elem[a], STEREO ? mark_of(a) : 0u, put);
        for (unsigned s = off[a]; s < off[a + 1]; ++s) {
            const unsigned e = raw[s], n = entry_nbr(e), r = rnum[s];
            if (e & SLOT_TREE) continue;
            if (pos[n] > p) {
                const char c = bond_symbol(entry_word(e), aromatic && info_aromatic(info[n]));
                if (c) put(c);
            }
            if (r >= 10) { put('%'); put((char)('0' + r / 10)); }
            put((char)('0' + r % 10));
        }
        for (unsigned k = 0; k < closes[a]; ++k) put(')');
    };

    // ---- positions: SM_PER neighbouring pieces per thread, one scan ----
    unsigned len[SM_PER], sum = 0, total;
#pragma unroll
    for (int q = 0; q < SM_PER; ++q) {
        unsigned l = 0;
        if (SM_PER * tid + q < na) piece((unsigned)(SM_PER * tid + q), [&](char) { ++l; });
        len[q] = l;
        sum += l;
    }
    unsigned at_byte = block_scan_excl<SM_THREADS>(sum, scan, &total);
    if (!FILL) {
        if (SYM && MARKS != 0u) sym_dropped = __syncthreads_or(sym_dropped);
        const unsigned symmetric = SYM && sym_dropped ? MNX_SMILES_SYM_DROPPED : 0u;
        const unsigned stereo = STEREO ? (dropped ? MNX_SMILES_WEDGES_DROPPED : 0u) | (marked ? MNX_SMILES_STEREO : 0u) |
                                             (unresolved ? MNX_SMILES_STEREO_UNRESOLVED : 0u)
                                       : wedge ? MNX_SMILES_WEDGES_DROPPED : 0u;
        const unsigned ez = (directed ? MNX_SMILES_EZ : 0u) | (ez_unresolved ? MNX_SMILES_EZ_UNRESOLVED : 0u) |
                            (implied ? MNX_SMILES_EZ_IMPLIED : 0u);
        record(total, base_flags | (pseudo ? PT_PSEUDO_ATOM : 0u) | stereo | ez | symmetric | (any ? MNX_SMILES_UNKNOWN_BOND : 0u), n_rings);
        return;
    }
#pragma unroll
    for (int q = 0; q < SM_PER; ++q) {
        if (SM_PER * tid + q >= na) break;
        unsigned long long o = (unsigned long long)text0 + at_byte;
        piece((unsigned)(SM_PER * tid + q), [&](char c) {                // nothing is written beyond out_cap
            if (o < out_cap) out[o] = c;
            ++o;
        });
        at_byte += len[q];
    }
    if (order)
        for (int a = tid; a < na; a += SM_THREADS) order[m.atom0 + a] = pos[a];
    if (SYM && atom_marks)                                // MNX_ATOM_MARK_CW / _CCW / _SYM are the bits of stk
        for (int a = tid; a < na; a += SM_THREADS) {
            const unsigned r = EZ ? done_last[a] : 0u;
            atom_marks[m.atom0 + a] = (unsigned char)((STEREO ? stk[a] & 7u : 0u) | (r & (ROLE_A | ROLE_B) ? MNX_ATOM_EZ : 0u) |
                                                      (r & ROLE_SYM ? MNX_ATOM_EZ_SYM : 0u));
        }
}

// the kernel of a set of marks
template <bool FILL, bool CANON, bool SYM = false>
auto smiles_kernel_for(unsigned marks) {
    return marks == 3u ? smiles_kernel<FILL, 3u, CANON, SYM> : marks == 2u ? smiles_kernel<FILL, 2u, CANON, SYM>
         : marks == 1u ? smiles_kernel<FILL, 1u, CANON, SYM> : smiles_kernel<FILL, 0u, CANON, SYM>;
}

}  // namespace

hipError_t smiles_pack_enqueue(const SymbolTables* st_dev, const PackedTables& t, unsigned marks, mnx_smiles* recs,
                               unsigned short* order, unsigned short* rank, unsigned short* sym_class, char* out,
                               unsigned out_cap, unsigned* totals, hipStream_t s, bool symmetric, unsigned char* atom_marks) {
    const bool canon = rank != nullptr;
    const auto count = symmetric ? smiles_kernel_for<false, true, true>(marks)
                     : canon ? smiles_kernel_for<false, true>(marks) : smiles_kernel_for<false, false>(marks);
    const auto fill = symmetric ? smiles_kernel_for<true, true, true>(marks)
                    : canon ? smiles_kernel_for<true, true>(marks) : smiles_kernel_for<true, false>(marks);
    if (canon) hipLaunchKernelGGL(canon_rank_kernel, dim3(t.n), dim3(SM_THREADS), 0, s, t, st_dev, recs, rank, sym_class);
    hipLaunchKernelGGL(count, dim3(t.n), dim3(SM_THREADS), 0, s, t, st_dev, recs, order, out, out_cap, rank, sym_class, atom_marks);
    hipLaunchKernelGGL(text_scan_kernel<mnx_smiles>, dim3(1), dim3(TEXT_SCAN_THREADS), 0, s, recs, t.n, out_cap, totals);
    hipLaunchKernelGGL(fill, dim3(t.n), dim3(SM_THREADS), 0, s, t, st_dev, recs, order, out, out_cap, rank, sym_class, atom_marks);
    return hipGetLastError();
}

}  // namespace mnx
