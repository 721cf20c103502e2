// grow_pass.h — the frame of a pass that replaces labels by atoms and bonds on the packed molecule tables (expand.hip,
// formula.hip), once (internal): packed tables in, packed tables of the same record types out. The molecule's own atoms keep
// their indices; a label's first atom takes the label's place, its other atoms follow behind the molecule's own; its bonds from
// the first atom go behind the bond records of the label's row, the others behind all own-row bonds. One workgroup of GR_THREADS
// per molecule, run twice (count, fill; tables_out.h). A pass says which atoms are labels, their five sizes, and a label's atoms,
// symbols and bonds; who is admitted and what a refusal leaves (table_pass.h), the check of the bond records, where everything
// goes and the molecule's own records are here. Every position follows from five prefix scans over the atoms and, for a
// label's own row, from a binary search in the bond records, which are sorted by i: no atomics, the output is the same word for
// word on every run.
#pragma once
#include "table_pass.h"

namespace mnx {

constexpr int GR_THREADS = 256;
constexpr int GR_MAX = 2048;             // atoms of a molecule held in LDS: 2047 atoms x 32 atoms of a label fit a uint16 index
constexpr int GR_PER = GR_MAX / GR_THREADS;
constexpr unsigned GR_ATOM_LIMIT = 2047;

// the five sizes of an atom, in the order of their scans: atoms appended behind the molecule's own (a label's atoms 1 .. m - 1);
// a label's bonds from its first atom, which go to the atom's own row; its bonds among the appended atoms; bytes of the atom's
// own symbol in the new text (the first atom's for a label); bytes of the appended atoms' symbols
enum { GR_ATOMS, GR_B0, GR_BIN, GR_TEXT, GR_MORE, GR_SIZES };

// Molecule blockIdx.x in one workgroup of a growing pass, count (FILL = false) or fill. The five arrays — per atom, what lies in
// front of it of each size — are the pass's, GR_MAX entries each in fill and unused in count; OFF is the element type of the first
// three, as narrow as the pass's labels allow.
template <bool FILL, typename OFF>
struct GrowPass : TablePass<FILL> {
    using P = TablePass<FILL>;
    using P::o; using P::mo; using P::na; using P::nb; using P::A; using P::B;
    OFF *const off_atoms, *const off_b0, *const off_bin;
    unsigned *const off_text, *const off_more;
    unsigned short* const origin;         // per output atom, the input atom it came from (or null)
    unsigned total[GR_SIZES];             // place(): the molecule's sum of each size

    __device__ __forceinline__ GrowPass(const PackedTables& t, const TablesOut& o, unsigned refused, unsigned short* origin,
                                        OFF* off_atoms, OFF* off_b0, OFF* off_bin, unsigned* off_text, unsigned* off_more)
        : P(t, o, refused), off_atoms(off_atoms), off_b0(off_b0), off_bin(off_bin), off_text(off_text), off_more(off_more),
          origin(origin) {}
    // too large: more atoms than GR_MAX holds with one to spare; no limit on bonds
    __device__ __forceinline__ bool admitted() { return P::admitted(P::mol.m.n_atoms > GR_ATOM_LIMIT); }

    // count: a bond that is no bond of the molecule, or bond records that are not sorted by i (the position of a label's new bonds
    // is found by a search in them), refuse the molecule as a symbol beyond the text (bad) does; one barrier
    __device__ __forceinline__ bool bonds_refuse(int bad) const {
        for (unsigned k = threadIdx.x; k < nb; k += GR_THREADS) {
            const BondEnds e = P::bond(k);
            if (e.beyond || (k > 0 && P::bond(k - 1).i > e.i)) bad = 1;
        }
        return P::refuses(bad);
    }

    // Placement: v[c][q] is size c of atom GR_PER * threadIdx.x + q. Five block scans (scan: 2 * GR_THREADS words of LDS), the
    // sums into total[], and in fill the exclusive offsets into the five arrays, behind a barrier.
    __device__ __forceinline__ void place(const unsigned (&v)[GR_SIZES][GR_PER], unsigned* scan) {
        unsigned e[GR_SIZES];
#pragma unroll
        for (int c = 0; c < GR_SIZES; ++c) {
            unsigned s = 0;
#pragma unroll
            for (int q = 0; q < GR_PER; ++q) s += v[c][q];
            e[c] = block_scan_excl<GR_THREADS>(s, scan, &total[c]);
        }
        if (!FILL) return;
#pragma unroll
        for (int q = 0; q < GR_PER; ++q) {
            const int a = GR_PER * threadIdx.x + q;
            off_atoms[a] = (OFF)e[GR_ATOMS]; off_b0[a] = (OFF)e[GR_B0]; off_bin[a] = (OFF)e[GR_BIN];
            off_text[a] = e[GR_TEXT]; off_more[a] = e[GR_MORE];
#pragma unroll
            for (int c = 0; c < GR_SIZES; ++c) e[c] += v[c][q];
        }
        __syncthreads();
    }

    // ---- fill, behind place(): where the records of the label at atom a go ----
    __device__ __forceinline__ unsigned first(unsigned a) const { return (unsigned)na + off_atoms[a]; }         // new index of its atom 1
    __device__ __forceinline__ unsigned more(unsigned a) const { return total[GR_TEXT] + off_more[a]; }        // byte of atom 1's symbol
    // its bonds from the first atom: behind the bond records of row a
    __device__ __forceinline__ unsigned row(unsigned a) const {
        unsigned lo = 0, hi = nb;                                    // first record with i > a
        while (lo < hi) {
            const unsigned mid = lo + ((hi - lo) >> 1);
            if (((unsigned)B[2 * (size_t)mid] & 0xffffu) <= a) lo = mid + 1; else hi = mid;
        }
        return lo + off_b0[a];
    }
    __device__ __forceinline__ unsigned inner(unsigned a) const { return nb + total[GR_B0] + off_bin[a]; }   // the others: behind all rows

    // ---- fill: capped stores behind the molecule's offsets ----
    // atom k of the new molecule, its symbol of sym_len bytes at byte sym0 of the new text (the bytes are written apart): index,
    // bins and score of the input record w0..w2
    __device__ __forceinline__ void put_record(unsigned k, unsigned sym0, unsigned sym_len, unsigned long long w0,
                                               unsigned long long w1, unsigned long long w2, unsigned from) const {
        const unsigned long long at = (unsigned long long)mo.atom0 + k;
        if (put_atom(o, at, atom_word0(sym0, sym_len, 0u) | (w0 & ATOM_INDEX_BITS), w1 & ATOM_BINS_BITS, w2) && origin)
            origin[at] = (unsigned short)from;
    }
    // atom a of the molecule's own, as it is: it keeps its index
    __device__ __forceinline__ void put_own_atom(int a) const {
        const unsigned long long w0 = A[3 * (size_t)a], w1 = A[3 * (size_t)a + 1], w2 = A[3 * (size_t)a + 2];
        const unsigned sl = (unsigned)(w0 >> 32) & 0xffffu;
        put_record((unsigned)a, off_text[a], sl, w0, w1, w2, (unsigned)a);
        put_text(o, (unsigned long long)mo.text0 + off_text[a], P::text_in() + (unsigned)w0, sl);
    }
    // bond k of the new molecule, one of a label's: i - j of type ty both ways, with the score word of the label's atom
    __device__ __forceinline__ void put_new_bond(unsigned k, unsigned i, unsigned j, unsigned ty, unsigned long long score) const {
        put_bond(o, (unsigned long long)mo.bond0 + k, bond_word0(i, j, ty, ty), score);
    }
    // the molecule's own bonds, each moved back by the new bonds of the rows in front of its own
    __device__ __forceinline__ void own_bonds() const {
        for (unsigned k = threadIdx.x; k < nb; k += GR_THREADS) {
            const unsigned long long w0 = B[2 * (size_t)k], w1 = B[2 * (size_t)k + 1];
            put_bond(o, (unsigned long long)mo.bond0 + k + off_b0[(unsigned)w0 & (GR_MAX - 1)], w0 & BOND_FIELD_BITS, w1);
        }
    }
};

}  // namespace mnx
