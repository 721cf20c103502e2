// kekulize.hip — aromatic systems of the packed molecule tables written as Kekule structures (mnx_kekulize_pack): the inverse of
// what normalize.hip perceives. Packed tables in, packed tables of the same record types out, atom and bond counts and order
// unchanged. The rule stands in include/molnextr_hip.h: a Kekule structure is a perfect matching of the atoms that must take a
// double bond, and the choice among several is this library's own search order, not a toolkit's.
//   count  one workgroup per molecule: systems, matchings, the bytes of the new text -> mols_out[b]
//   scan   exclusive scan of the three counts over the molecules -> atom0 / bond0 / text0, totals (tables_out.h)
//   fill   one workgroup per molecule: the same again, the records behind those offsets
// Inside a workgroup: the atoms' interpretation (atom_symbol.h); one stride over the bond records for every atom's bond order sum,
// its type-4 records (the first three as a neighbour list) and the pair of every record as a sort key; a bitonic sort of the keys,
// so that two records of one pair lie side by side; the systems by label propagation over the type-4 records between aromatic
// atoms, with pointer jumping; the needy neighbours of every needy atom; then ONE LANE PER SYSTEM runs the search of
// kekule_search.h, the systems of a molecule side by side, everything in LDS; then every atom's new symbol, placed by a prefix
// scan. LDS atomics count, add up, hand out the slots of a list that is sorted afterwards, set bits of sets and take the minimum
// of a set: no atomic decides a position, an order or a result.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/molnextr_hip.h"
#include "atom_spell.h"
#include "atom_symbol.h"
#include "dec_types.h"
#include "kekule_search.h"
#include "tables_out.h"

namespace mnx {
namespace {

constexpr int KK_THREADS = 256;
constexpr int KK_MAX = 1024;             // atoms and bond records held in LDS (999 at most)
constexpr int KK_PER = KK_MAX / KK_THREADS;
constexpr unsigned KK_NONE = 0xFFFFFFFFu;
static_assert(kekule::NONE >= 999u && kekule::NONE < (unsigned)KK_MAX, "an atom index that no atom has, in 10 bits");

// ---- an atom's state word ----
//   bits 0-3 H count, bit 4 aromatic atom, bit 5 needy, bit 6 one of the atom's records blocks its system,
//   on a system's lowest atom: bit 7 the system is blocked, bits 8-9 what the search returned (kekule::OK / NO_MATCHING / LIMIT)
constexpr unsigned ST_AROMATIC = 1u << 4, ST_NEEDY = 1u << 5, ST_BLOCKS = 1u << 6, ST_BLOCKED = 1u << 7, ST_RESULT = 8;
__device__ __forceinline__ unsigned st_h(unsigned s) { return s & 15u; }
__device__ __forceinline__ unsigned st_result(unsigned s) { return s >> ST_RESULT & 3u; }

// v of the needy rule for (element, charge); 0 for a pair the rule does not list
__device__ __forceinline__ unsigned needy_valence(unsigned el, int q) {
    if (el == EL('C')) return q == 0 ? 4u : (q == 1 || q == -1) ? 3u : 0u;
    if (el == EL('N') || el == EL('P')) return q == 0 ? 3u : q == 1 ? 4u : 0u;
    if (el == EL('B')) return q == 0 ? 3u : q == -1 ? 4u : 0u;
    if (el == EL('A', 's')) return q == 0 ? 3u : 0u;
    if (el == EL('O') || el == EL('S') || el == EL('S', 'e')) return q == 0 ? 2u : q == 1 ? 3u : 0u;
    return 0u;
}

template <bool FILL>
__global__ __launch_bounds__(KK_THREADS) void kekulize_kernel(
        const PackedTables t, const SymbolTables* __restrict__ stab, const TablesOut o, unsigned char* __restrict__ notes,
        const unsigned max_steps) {
    __shared__ unsigned info[KK_MAX], elem[KK_MAX];
    __shared__ unsigned cnt[KK_MAX];      // type-4 records at the atom: hands out the slots of nbr3
    __shared__ unsigned acc[KK_MAX];      // bond order sum
    __shared__ unsigned st[KK_MAX];
    __shared__ unsigned nbr3[3 * KK_MAX]; // the first three type-4 neighbours; later the needy neighbours of a needy atom
    __shared__ unsigned keys[KK_MAX];     // per bond record: lower atom << 10 | higher atom, sorted
    __shared__ unsigned edge[KK_MAX];     // per bond record: i | j << 10 of a type-4 record between two aromatic atoms, else KK_NONE
    __shared__ unsigned label[KK_MAX];    // an aromatic atom's system: the lowest atom of its component
    __shared__ unsigned searched[KK_MAX]; // the system a needy atom is searched in, kekule::NONE for every other atom
    __shared__ unsigned state[KK_MAX];    // the search's word per needy atom (kekule_search.h)
    __shared__ unsigned scan[2 * KK_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const Molecule mol = admit_molecule(t, b);
    const mnx_mol& m = mol.m;
    auto record = [&](unsigned n_atoms, unsigned n_bonds, unsigned text_len, unsigned flags) {      // count's result
        if (tid == 0) store_mol_counts(&o.mols[b], n_atoms, n_bonds, text_len, flags | (m.flags & MNX_MOL_TRUNCATED), m.overall_score);
    };
    mnx_mol mo;
    if (FILL) {
        mo = o.mols[b];
        if (mo.flags & MNX_MOL_KEKULIZE_REFUSED) return;    // refused by count (the same for every thread)
    } else if (mol.flags & (PT_BEYOND_TABLES | PT_TOO_LARGE)) {
        record(0, 0, 0, MNX_MOL_KEKULIZE_REFUSED);
        return;
    }
    const int na = (int)m.n_atoms, nb = (int)m.n_bonds;
    const unsigned long long* A = (const unsigned long long*)mol.A;
    const unsigned long long* B = (const unsigned long long*)mol.B;

    // ---- the atoms as the writers read them; per atom its bond order sum and its first three type-4 records ----
    int bad = interpret_atoms<KK_MAX, KK_THREADS>(t, stab, mol, info, elem);
    for (int a = tid; a < KK_MAX; a += KK_THREADS) {
        cnt[a] = 0; acc[a] = 0; st[a] = 0;
        nbr3[3 * a] = nbr3[3 * a + 1] = nbr3[3 * a + 2] = KK_NONE;
        keys[a] = KK_NONE; edge[a] = KK_NONE; label[a] = KK_NONE; searched[a] = kekule::NONE;
    }
    __syncthreads();
    auto aromatic_atom = [&](unsigned a) { return info_cls(info[a]) == CLS_ATOM && info_aromatic(info[a]); };
    int any = 0;
    for (int a = tid; a < na; a += KK_THREADS) any |= aromatic_atom((unsigned)a);
    for (int k = tid; k < nb; k += KK_THREADS) {
        const unsigned w = (unsigned)B[2 * (size_t)k], i = w & 0xffffu, j = w >> 16, ty = (unsigned)(B[2 * (size_t)k] >> 32) & 0xffu;
        if (i >= (unsigned)na || j >= (unsigned)na) { bad = 1; continue; }
        const unsigned order = (ty == 1 || ty == 4 || ty == 5 || ty == 6) ? 1u : (ty == 2 || ty == 3) ? ty : 0u;
        unsigned fi = (order == 0 || i == j) ? ST_BLOCKS : 0u, fj = fi;     // no class of a bond, or from an atom to itself
        if (ty == 4 && i != j) {
            const bool ai = aromatic_atom(i), aj = aromatic_atom(j);
            if (!aj) fi |= ST_BLOCKS;     // the other end is no aromatic atom
            if (!ai) fj |= ST_BLOCKS;
            if (ai && aj) edge[k] = i | j << 10;
            const unsigned si = atomicAdd(&cnt[i], 1u), sj = atomicAdd(&cnt[j], 1u);    // any slot: the three are sorted below
            if (si < 3) nbr3[3 * i + si] = j;
            if (sj < 3) nbr3[3 * j + sj] = i;
        }
        if (fi) atomicOr(&st[i], fi);
        if (fj) atomicOr(&st[j], fj);
        atomicAdd(&acc[i], order);        // a sum does not depend on the order of its terms; a record from an atom to itself
        atomicAdd(&acc[j], order);        // counts at both of its ends
        keys[k] = min(i, j) << 10 | max(i, j);
    }
    bad = __syncthreads_or(bad);
    if (!FILL && bad) {                   // a symbol beyond the text or a bond that is no bond of the molecule
        record(0, 0, 0, MNX_MOL_KEKULIZE_REFUSED);
        return;
    }
    any = __syncthreads_or(any);

    if (any) {                            // the same for every thread; without an aromatic atom everything is copied
        // ---- two records of one pair of atoms: side by side behind a bitonic sort of the keys ----
        int width = 2;
        while (width < nb) width <<= 1;
        for (int run = 2; run <= width; run <<= 1)
            for (int d = run >> 1; d > 0; d >>= 1) {
                for (int x = tid; x < width; x += KK_THREADS) {
                    const int y = x ^ d;
                    if (y > x) {
                        const unsigned p = keys[x], q = keys[y];
                        if ((p > q) == ((x & run) == 0)) { keys[x] = q; keys[y] = p; }
                    }
                }
                __syncthreads();
            }
        for (int x = tid; x + 1 < width; x += KK_THREADS) {
            const unsigned p = keys[x];
            if (p != KK_NONE && p == keys[x + 1]) {
                atomicOr(&st[p >> 10], ST_BLOCKS);
                atomicOr(&st[p & 1023u], ST_BLOCKS);
            }
        }
        __syncthreads();

        // ---- every aromatic atom: hydrogens, whether it is needy, its three slots in ascending order, a system of its own ----
        for (int a = tid; a < na; a += KK_THREADS) {
            if (!aromatic_atom((unsigned)a)) { st[a] = 0; continue; }
            const unsigned w = info[a], el = elem[a] & 0xffffu, bo = acc[a];
            unsigned e0 = nbr3[3 * a], e1 = nbr3[3 * a + 1], e2 = nbr3[3 * a + 2], x;
            if (e0 > e1) { x = e0; e0 = e1; e1 = x; }
            if (e1 > e2) { x = e1; e1 = e2; e2 = x; }
            if (e0 > e1) { x = e0; e0 = e1; e1 = x; }
            nbr3[3 * a] = e0; nbr3[3 * a + 1] = e1; nbr3[3 * a + 2] = e2;
            const unsigned h = (w & 4u) ? (unsigned)info_h(w) : el == EL('C') ? (bo < 3 ? 3 - bo : 0u) : 0u;
            const unsigned v = needy_valence(el, info_charge(w));
            const bool needy = v != 0 && v == bo + h + 1;
            st[a] = h | ST_AROMATIC | (needy ? ST_NEEDY : 0u) | ((st[a] & ST_BLOCKS) || cnt[a] > 3 ? ST_BLOCKS : 0u);
            label[a] = (unsigned)a;
        }
        __syncthreads();

        // ---- systems: every atom's label falls to the lowest atom of its component; a label is always an atom of the component,
        //      so the minimum the atomics take is the same whatever their order. At most one round per atom, a few in practice ----
        for (int round = 0; round < KK_MAX; ++round) {
            int changed = 0;
            for (int k = tid; k < nb; k += KK_THREADS) {
                const unsigned e = edge[k];
                if (e == KK_NONE) continue;
                const unsigned i = e & 1023u, j = e >> 10, li = label[i], lj = label[j];
                if (li < lj) { atomicMin(&label[j], li); changed = 1; }
                else if (lj < li) { atomicMin(&label[i], lj); changed = 1; }
            }
            __syncthreads();
            for (int a = tid; a < na; a += KK_THREADS) {
                const unsigned l = label[a];
                if (l == KK_NONE) continue;
                const unsigned ll = label[l];
                if (ll < l) { atomicMin(&label[a], ll); changed = 1; }
            }
            if (!__syncthreads_or(changed)) break;
        }
        for (int a = tid; a < na; a += KK_THREADS)
            if ((st[a] & (ST_AROMATIC | ST_BLOCKS)) == (ST_AROMATIC | ST_BLOCKS)) atomicOr(&st[label[a]], ST_BLOCKED);
        __syncthreads();

        // ---- a needy atom of a system that is not blocked: the system it is searched in and its needy neighbours, ascending. All
        //      its type-4 records are in its three slots, go to aromatic atoms of its system and to different ones ----
        for (int a = tid; a < na; a += KK_THREADS) {
            const unsigned s = st[a];
            const bool in = (s & ST_NEEDY) && !(st[label[a]] & ST_BLOCKED);
            unsigned e[3] = {kekule::NONE, kekule::NONE, kekule::NONE}, n = 0;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const unsigned x = nbr3[3 * a + q];
                const bool keep = in && x != KK_NONE && (st[x] & ST_NEEDY);
                if (keep && n == 0) e[0] = x;
                if (keep && n == 1) e[1] = x;
                if (keep && n == 2) e[2] = x;
                n += keep;
            }
            nbr3[3 * a] = e[0]; nbr3[3 * a + 1] = e[1]; nbr3[3 * a + 2] = e[2];
            if (in) searched[a] = label[a];
        }
        __syncthreads();

        // ---- the search: one lane per system that is not blocked, serial inside a system ----
        for (int a = tid; a < na; a += KK_THREADS) {
            const unsigned s = st[a];
            if (!(s & ST_AROMATIC) || label[a] != (unsigned)a || (s & ST_BLOCKED)) continue;
            unsigned steps;
            st[a] = s | kekule::search((unsigned)a, (unsigned)na, searched, nbr3, state, max_steps, &steps) << ST_RESULT;
        }
        __syncthreads();
    }

    // whether the aromatic atom a was rewritten: its system is not blocked and has a matching
    auto rewritten = [&](unsigned a) {
        const unsigned sr = st[label[a]];
        return !(sr & ST_BLOCKED) && st_result(sr) == kekule::OK;
    };

    // ---- every atom's new symbol: KK_PER neighbouring atoms per thread, placed by a prefix scan over their lengths ----
    const unsigned char* text_in = t.text + m.text0;
    unsigned long long sym8[KK_PER];      // a respelled symbol's bytes 0-7 (the first in the low byte) and 8-11
    unsigned sym4[KK_PER], len[KK_PER], note[KK_PER], sum = 0;
    int any_done = 0, any_left = 0;
#pragma unroll
    for (int q = 0; q < KK_PER; ++q) {
        const int a = KK_PER * tid + q;
        sym8[q] = 0; sym4[q] = 0; len[q] = 0; note[q] = 0;
        if (a >= na) continue;
        const unsigned s = st[a], w = info[a];
        if (!(s & ST_AROMATIC) || !rewritten((unsigned)a)) {
            if (!(s & ST_AROMATIC)) note[q] = MNX_NOTE_COPIED;
            else {
                const unsigned sr = st[label[a]];
                note[q] = st_h(s) | MNX_NOTE_KEKULE_LEFT | (!(sr & ST_BLOCKED) && st_result(sr) == kekule::LIMIT ? MNX_NOTE_KEKULE_LIMIT : 0u);
                any_left = 1;
            }
            len[q] = (unsigned)(A[3 * (size_t)a] >> 32) & 0xffffu;
            sum += len[q];
            continue;
        }
        const unsigned el = elem[a] & 0xffffu, bo = acc[a] + ((s & ST_NEEDY) ? 1u : 0u);     // a needy atom took one double bond
        unsigned n = 0;
        unsigned long long lo = 0;
        unsigned hi = 0;
        spell_atom(el, false, info_num(w), st_h(s), info_charge(w), implicit_h(el, bo), [&](char c) {
            if (n < 8u) lo |= (unsigned long long)(unsigned char)c << (8u * n);
            else if (n < 12u) hi |= (unsigned)(unsigned char)c << (8u * (n - 8u));
            ++n;
        });
        sym8[q] = lo; sym4[q] = hi; len[q] = n; sum += n;
        note[q] = st_h(s) | MNX_NOTE_KEKULIZED;
        any_done = 1;
    }
    unsigned total;
    unsigned at = block_scan_excl<KK_THREADS>(sum, scan, &total);
    if (!FILL) {
        any_done = __syncthreads_or(any_done);
        any_left = __syncthreads_or(any_left);
        record((unsigned)na, (unsigned)nb, total, (any_done ? MNX_MOL_KEKULIZED : 0u) | (any_left ? MNX_MOL_KEKULE_LEFT : 0u));
        return;
    }
#pragma unroll
    for (int q = 0; q < KK_PER; ++q) {
        const int a = KK_PER * tid + q;
        if (a >= na) continue;
        const unsigned long long w0 = A[3 * (size_t)a], w1 = A[3 * (size_t)a + 1], w2 = A[3 * (size_t)a + 2];
        const unsigned long long rec = (unsigned long long)mo.atom0 + (unsigned)a, to = (unsigned long long)mo.text0 + at;
        if (put_atom(o, rec, atom_word0(at, len[q], 0u) | (w0 & ATOM_INDEX_BITS), w1 & ATOM_BINS_BITS, w2) && notes)
            notes[rec] = (unsigned char)note[q];
        if (!(note[q] & MNX_NOTE_KEKULIZED)) put_text(o, to, text_in + (unsigned)w0, len[q]);
        else
            for (unsigned c = 0; c < len[q]; ++c)
                if (to + c < o.text_cap) o.text[to + c] = (char)(c < 8u ? sym8[q] >> (8u * c) : (unsigned long long)(sym4[q] >> (8u * (c - 8u))));
        at += len[q];
    }
    // ---- the bonds: a type-4 record of a rewritten system is double between partners and single otherwise ----
    for (int k = tid; k < nb; k += KK_THREADS) {
        unsigned long long w0 = B[2 * (size_t)k] & BOND_FIELD_BITS;
        const unsigned e = edge[k];
        if (e != KK_NONE && rewritten(e & 1023u)) {
            const unsigned i = e & 1023u, j = e >> 10;
            const unsigned long long ty = (st[i] & ST_NEEDY) && kekule::partner(state[i]) == j ? 2ull : 1ull;
            w0 = (w0 & 0xffffffffull) | ty << 32 | ty << 40;
        }
        put_bond(o, (unsigned long long)mo.bond0 + (unsigned)k, w0, B[2 * (size_t)k + 1]);
    }
}

}  // namespace

hipError_t kekulize_pack_enqueue(const SymbolTables* st_dev, const PackedTables& t, const TablesOut& o, unsigned char* atom_notes,
                                 unsigned* totals, unsigned max_steps, hipStream_t s) {
    const unsigned steps = max_steps ? max_steps : MNX_KEKULE_DEFAULT_STEPS;
    hipLaunchKernelGGL(kekulize_kernel<false>, dim3(t.n), dim3(KK_THREADS), 0, s, t, st_dev, o, atom_notes, steps);
    hipLaunchKernelGGL(mol_scan_kernel, dim3(1), dim3(MOL_SCAN_THREADS), 0, s, o, t.n, totals);
    hipLaunchKernelGGL(kekulize_kernel<true>, dim3(t.n), dim3(KK_THREADS), 0, s, t, st_dev, o, atom_notes, steps);
    return hipGetLastError();
}

}  // namespace mnx
