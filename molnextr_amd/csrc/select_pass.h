// select_pass.h — the frame of a pass that drops atoms from the packed molecule tables (main_mol.hip), once (internal): packed
// tables in, packed tables of the same record types out. A pass says which atoms stay (a keep mask); the kept atoms take new
// indices in ascending old index, their symbols go behind one another in the new text, a bond record stays iff its i stays (the
// pass vouches that its j stays then) and keeps its place among the kept records, its ends renumbered. One workgroup of
// SEL_THREADS per molecule, run twice (count, fill; tables_out.h). Who is admitted and what a refusal leaves is table_pass.h's;
// the check of the records, the scans that turn the mask into new indices and text offsets, and the capped stores of what stays
// are here. Every position follows from a prefix scan — over the atoms, SEL_PER neighbours per thread, and over the bond records
// in tiles of the workgroup with a running carry: no atomics, the output is the same word for word on every run. The bond records
// need not be sorted; a sorted table stays sorted.
#pragma once
#include "table_pass.h"

namespace mnx {

constexpr int SEL_THREADS = 256;
constexpr int SEL_MAX = 2048;            // atoms of a molecule held in LDS, as grow_pass.h
constexpr int SEL_PER = SEL_MAX / SEL_THREADS;
constexpr unsigned SEL_ATOM_LIMIT = 2047;
constexpr unsigned SEL_DROPPED = 0xffffu;    // new_index of an atom that does not stay

// Molecule blockIdx.x in one workgroup of a selecting pass, count (FILL = false) or fill. new_index is the pass's, SEL_MAX entries
// of LDS in count and fill: behind place_atoms() the new index of an atom that stays, SEL_DROPPED for every other one.
template <bool FILL>
struct SelectPass : TablePass<FILL> {
    using P = TablePass<FILL>;
    using P::o; using P::mo; using P::na; using P::nb; using P::A; using P::B;
    unsigned short* const new_index;
    unsigned short* const origin;         // per output atom, the input atom it was (or null)
    unsigned n_atoms, n_text, n_bonds;    // what stays: place_atoms() the first two, place_bonds() the third

    __device__ __forceinline__ SelectPass(const PackedTables& t, const TablesOut& o, unsigned refused, unsigned short* origin,
                                          unsigned short* new_index)
        : P(t, o, refused), new_index(new_index), origin(origin), n_atoms(0), n_text(0), n_bonds(0) {}
    // too large: more atoms than SEL_MAX holds with one to spare; no limit on bonds
    __device__ __forceinline__ bool admitted() { return P::admitted(P::mol.m.n_atoms > SEL_ATOM_LIMIT); }

    // count: a symbol beyond the text or a bond that is no bond of the molecule refuses it; one barrier. Behind it every i and j
    // of a bond record indexes the molecule's atoms.
    __device__ __forceinline__ bool records_refuse() const {
        int bad = 0;
        for (int a = threadIdx.x; a < na; a += SEL_THREADS) {
            const unsigned long long w0 = A[3 * (size_t)a];
            if ((unsigned long long)P::mol.m.text0 + (unsigned)w0 + ((unsigned)(w0 >> 32) & 0xffffu) > P::t.n_text_bytes) bad = 1;
        }
        for (size_t k = threadIdx.x; k < nb; k += SEL_THREADS)
            if (P::bond(k).beyond) bad = 1;
        return P::refuses(bad);
    }

    // The atoms: keep[q] says whether atom SEL_PER * threadIdx.x + q stays (false at and beyond n_atoms). Two block scans (scan:
    // 2 * SEL_THREADS words of LDS) give n_atoms and n_text and every atom's new_index; fill stores the kept records with their
    // index, bins and score, sym0 / sym_len naming the new span, the symbol's bytes and origin. Ends with a barrier.
    __device__ __forceinline__ void place_atoms(const bool (&keep)[SEL_PER], unsigned* scan) {
        unsigned long long w0[SEL_PER];
        unsigned atoms = 0, bytes = 0;
#pragma unroll
        for (int q = 0; q < SEL_PER; ++q) {
            w0[q] = keep[q] ? A[3 * (size_t)(SEL_PER * threadIdx.x + q)] : 0ull;
            atoms += keep[q] ? 1u : 0u;
            bytes += (unsigned)(w0[q] >> 32) & 0xffffu;
        }
        unsigned k = block_scan_excl<SEL_THREADS>(atoms, scan, &n_atoms);
        unsigned at = block_scan_excl<SEL_THREADS>(bytes, scan, &n_text);
#pragma unroll
        for (int q = 0; q < SEL_PER; ++q) {
            const int a = SEL_PER * threadIdx.x + q;
            new_index[a] = (unsigned short)(keep[q] ? k : SEL_DROPPED);
            if (!keep[q]) continue;
            const unsigned sl = (unsigned)(w0[q] >> 32) & 0xffffu;
            if (FILL) {
                const unsigned long long to = (unsigned long long)mo.atom0 + k;
                if (put_atom(o, to, atom_word0(at, sl, 0u) | (w0[q] & ATOM_INDEX_BITS), A[3 * (size_t)a + 1] & ATOM_BINS_BITS,
                             A[3 * (size_t)a + 2]) && origin)
                    origin[to] = (unsigned short)a;
                put_text(o, (unsigned long long)mo.text0 + at, P::text_in() + (unsigned)w0[q], sl);
            }
            ++k;
            at += sl;
        }
        __syncthreads();
    }

    // The bond records, behind place_atoms(): a record stays iff its i stays. count: n_bonds from one scan of the threads' sums.
    // fill: the kept records in input order, tile by tile with a running carry, i and j renumbered, type, rev and score as they are.
    __device__ __forceinline__ void place_bonds(unsigned* scan) {
        if (!FILL) {
            unsigned mine = 0;
            for (size_t k = threadIdx.x; k < nb; k += SEL_THREADS) mine += new_index[P::bond(k).i] != SEL_DROPPED ? 1u : 0u;
            block_scan_excl<SEL_THREADS>(mine, scan, &n_bonds);
            return;
        }
        unsigned carry = 0;
        for (unsigned long long base = 0; base < nb; base += SEL_THREADS) {
            const unsigned long long k = base + threadIdx.x;
            unsigned long long w0 = 0;
            unsigned i = SEL_DROPPED, j = SEL_DROPPED, tile;
            if (k < nb) {
                w0 = B[2 * k];
                i = new_index[(unsigned)w0 & 0xffffu];
                j = new_index[(unsigned)w0 >> 16];
            }
            const bool stays = i != SEL_DROPPED;
            const unsigned e = block_scan_excl<SEL_THREADS>(stays ? 1u : 0u, scan, &tile);
            if (stays)
                put_bond(o, (unsigned long long)mo.bond0 + carry + e, (w0 & BOND_FIELD_BITS & ~0xffffffffull) | i | (unsigned long long)j << 16,
                         B[2 * k + 1]);
            carry += tile;
        }
        n_bonds = carry;
    }
};

}  // namespace mnx
