// expand.hip — abbreviation labels replaced by their atoms and bonds (mnx_expand_pack): what the reference's
// _expand_functional_group does to an atom whose alias is in its abbreviation table before anything is written, here from a table
// of fragments (mnx_set_fragments) and on the packed molecule tables of mnx_graph_pack — packed tables in, packed tables of the
// same record types out, so that mnx_molfile_pack and the mnx_smiles_pack calls run on the expanded molecule unchanged.
//   count  one workgroup per molecule: which atoms are labels with a fragment (atom_symbol.h reads the symbol, as the writers
//          do), the atoms / bonds / text bytes of the expanded molecule -> mols_out[b]
//   scan   exclusive scan of the three counts over the molecules -> atom0 / bond0 / text0, totals (tables_out.h)
//   fill   one workgroup per molecule: the records behind those offsets
// The rule stands in include/molnextr_hip.h. Every position follows from a prefix scan over the atoms (the appended atoms of a
// label, the rows of the bond table, the bytes of the text) and, for a label's own row, from a binary search in the molecule's
// bond records, which are sorted by i: no atomics, the output is the same word for word on every run. Where a record's
// fields go is tables_out.h. The fragment tables are read from global memory (a few KB, shared by every
// workgroup of the launch).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/molnextr_hip.h"
#include "atom_symbol.h"
#include "dec_types.h"
#include "tables_out.h"

namespace mnx {
namespace {

constexpr int EX_THREADS = 256;
constexpr int EX_MAX = 2048;             // atoms of a molecule held in LDS: 2047 atoms x 32 fragment atoms fit a uint16 index
constexpr int EX_PER = EX_MAX / EX_THREADS;
constexpr unsigned EX_ATOM_LIMIT = 2047;

// what one atom adds to the expanded molecule
struct Grow {
    int frag;               // its fragment, -1: the atom stays as it is
    unsigned atoms;         // atoms appended behind the molecule's own (fragment atoms 1 .. m - 1)
    unsigned bonds0;        // fragment bonds from the attachment atom: they go to the atom's own row
    unsigned bonds_in;      // fragment bonds among the appended atoms
    unsigned text;          // bytes of the atom's own symbol in the new text (the attachment atom's for a label)
    unsigned text_more;     // bytes of the appended atoms' symbols
    bool left;              // a pseudo-atom that stays
};

// atom a of an admitted molecule; *bad is set when its symbol ends behind the text table
__device__ __forceinline__ Grow grow_of(const PackedTables& t, const SymbolTables* __restrict__ st, const FragView& fv,
                                        const Molecule& mol, int a, int* bad) {
    Grow g{-1, 0u, 0u, 0u, 0u, 0u, false};
    const unsigned s0 = mol.A[a].sym0, sl = mol.A[a].sym_len;
    if ((unsigned long long)mol.m.text0 + s0 + sl > t.n_text_bytes) { *bad = 1; return g; }
    unsigned s3;
    int name;
    const unsigned w = interpret_atom(st, t.text + mol.m.text0 + s0, (int)sl, &s3, &name);
    g.text = sl;
    if (info_cls(w) == CLS_ATOM) return g;
    if (info_cls(w) == CLS_PSEUDO && name >= 0 && st->kind[name] == 2) g.frag = fv.frag_of_name[name];
    if (g.frag < 0) { g.left = true; return g; }
    const FragRec f = fv.frag[g.frag];
    g.atoms = f.n_atoms - 1u;
    g.bonds0 = f.n_bonds0;
    g.bonds_in = (unsigned)f.n_bonds - f.n_bonds0;
    g.text = fv.atoms[f.atom0] >> 16;
    g.text_more = f.text_len - g.text;
    return g;
}

template <bool FILL>
__global__ __launch_bounds__(EX_THREADS) void expand_kernel(
        const PackedTables t, const SymbolTables* __restrict__ st, const FragView fv, const TablesOut o,
        unsigned short* __restrict__ origin) {
    // fill: per atom, what lies in front of it — appended atoms, bonds from attachment atoms, bonds among appended atoms, bytes
    // of the molecule's own atoms' symbols, bytes of the appended atoms' symbols
    __shared__ unsigned off_atoms[FILL ? EX_MAX : 1], off_b0[FILL ? EX_MAX : 1], off_bin[FILL ? EX_MAX : 1];
    __shared__ unsigned off_text[FILL ? EX_MAX : 1], off_more[FILL ? EX_MAX : 1];
    __shared__ short frag_of[FILL ? EX_MAX : 1];
    __shared__ unsigned scan[2 * EX_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const Molecule mol = admit_molecule(t, b);
    const mnx_mol& m = mol.m;
    auto record = [&](unsigned n_atoms, unsigned n_bonds, unsigned text_len, unsigned flags) {      // count's result
        if (tid == 0) store_mol_counts(&o.mols[b], n_atoms, n_bonds, text_len, flags | (m.flags & MNX_MOL_TRUNCATED), m.overall_score);
    };
    mnx_mol mo;
    if (FILL) {
        mo = o.mols[b];
        if (mo.flags & MNX_MOL_EXPAND_REFUSED) return;      // refused by count (the same for every thread)
    } else if ((mol.flags & PT_BEYOND_TABLES) || m.n_atoms > EX_ATOM_LIMIT) {
        record(0, 0, 0, MNX_MOL_EXPAND_REFUSED);
        return;
    }
    const int na = (int)m.n_atoms;
    const unsigned nb = m.n_bonds;
    const unsigned long long* A = (const unsigned long long*)mol.A;
    const unsigned long long* B = (const unsigned long long*)mol.B;

    // ---- every atom: EX_PER neighbouring atoms per thread ----
    int bad = 0, any = 0, left = 0;
    unsigned v_atoms[EX_PER], v_b0[EX_PER], v_bin[EX_PER], v_text[EX_PER], v_more[EX_PER];
    unsigned s_atoms = 0, s_b0 = 0, s_bin = 0, s_text = 0, s_more = 0;
#pragma unroll
    for (int q = 0; q < EX_PER; ++q) {
        const int a = EX_PER * tid + q;
        Grow g{-1, 0u, 0u, 0u, 0u, 0u, false};
        if (a < na) g = grow_of(t, st, fv, mol, a, &bad);
        if (FILL) frag_of[a] = (short)g.frag;
        any |= g.frag >= 0;
        left |= g.left;
        v_atoms[q] = g.atoms; v_b0[q] = g.bonds0; v_bin[q] = g.bonds_in; v_text[q] = g.text; v_more[q] = g.text_more;
        s_atoms += g.atoms; s_b0 += g.bonds0; s_bin += g.bonds_in; s_text += g.text; s_more += g.text_more;
    }
    unsigned t_atoms, t_b0, t_bin, t_text, t_more;
    unsigned e_atoms = block_scan_excl<EX_THREADS>(s_atoms, scan, &t_atoms);
    unsigned e_b0 = block_scan_excl<EX_THREADS>(s_b0, scan, &t_b0);
    unsigned e_bin = block_scan_excl<EX_THREADS>(s_bin, scan, &t_bin);
    unsigned e_text = block_scan_excl<EX_THREADS>(s_text, scan, &t_text);
    unsigned e_more = block_scan_excl<EX_THREADS>(s_more, scan, &t_more);

    if (!FILL) {
        // a bond that is no bond of the molecule, or bond records that are not sorted by i (the position of a label's new bonds
        // is found by a search in them), refuse the molecule as a symbol beyond the text does
        for (unsigned k = tid; k < nb; k += EX_THREADS) {
            const unsigned w = (unsigned)B[2 * (size_t)k], i = w & 0xffffu, j = w >> 16;
            if (i >= (unsigned)na || j >= (unsigned)na) bad = 1;
            if (k > 0 && ((unsigned)B[2 * (size_t)(k - 1)] & 0xffffu) > i) bad = 1;
        }
        const unsigned long long n_bonds = (unsigned long long)nb + t_b0 + t_bin;
        bad = __syncthreads_or(bad || n_bonds > 0xffffffffull);
        any = __syncthreads_or(any);
        left = __syncthreads_or(left);
        if (bad) record(0, 0, 0, MNX_MOL_EXPAND_REFUSED);
        else record((unsigned)na + t_atoms, (unsigned)n_bonds, t_text + t_more,
                    (any ? MNX_MOL_EXPANDED : 0u) | (left ? MNX_MOL_LABEL_LEFT : 0u));
        return;
    }
#pragma unroll
    for (int q = 0; q < EX_PER; ++q) {
        const int a = EX_PER * tid + q;
        off_atoms[a] = e_atoms; off_b0[a] = e_b0; off_bin[a] = e_bin; off_text[a] = e_text; off_more[a] = e_more;
        e_atoms += v_atoms[q]; e_b0 += v_b0[q]; e_bin += v_bin[q]; e_text += v_text[q]; e_more += v_more[q];
    }
    __syncthreads();

    const unsigned char* text_in = t.text + m.text0;
    // atom k of the new molecule, its symbol at byte sym0 of the new text: index, bins and score of the input record w0..w2
    auto atom = [&](unsigned k, unsigned sym0, const unsigned char* sym, unsigned sym_len, unsigned long long w0,
                    unsigned long long w1, unsigned long long w2, unsigned from) {
        const unsigned long long at = (unsigned long long)mo.atom0 + k;
        if (put_atom(o, at, atom_word0(sym0, sym_len, 0u) | (w0 & ATOM_INDEX_BITS), w1 & ATOM_BINS_BITS, w2) && origin)
            origin[at] = (unsigned short)from;
        put_text(o, (unsigned long long)mo.text0 + sym0, sym, sym_len);
    };
    auto bond = [&](unsigned k, unsigned long long w0, unsigned long long w1) {
        put_bond(o, (unsigned long long)mo.bond0 + k, w0 & BOND_FIELD_BITS, w1);
    };

    // ---- atoms and text: the molecule's own atoms keep their indices, a label's further atoms follow behind them ----
    for (int a = tid; a < na; a += EX_THREADS) {
        const unsigned long long w0 = A[3 * (size_t)a], w1 = A[3 * (size_t)a + 1], w2 = A[3 * (size_t)a + 2];
        const int fi = frag_of[a];
        if (fi < 0) {
            const unsigned sl = (unsigned)(w0 >> 32) & 0xffffu;
            atom((unsigned)a, off_text[a], text_in + (unsigned)w0, sl, w0, w1, w2, (unsigned)a);
            continue;
        }
        const FragRec f = fv.frag[fi];
        const unsigned len0 = fv.atoms[f.atom0] >> 16;
        const unsigned first = (unsigned)na + off_atoms[a];          // new index of fragment atom 1
        const unsigned more0 = t_text + off_more[a];                 // where the symbol of fragment atom 1 begins
        for (unsigned q = 0; q < f.n_atoms; ++q) {
            const unsigned fa = fv.atoms[f.atom0 + q], fs0 = fa & 0xffffu, fl = fa >> 16;
            const unsigned at = q == 0 ? off_text[a] : more0 + fs0 - len0;
            atom(q == 0 ? (unsigned)a : first + q - 1, at, fv.text + f.text0 + fs0, fl, w0, w1, w2, (unsigned)a);
        }
        // its bonds: those from the attachment atom behind the bond records of row a, the others in the rows of the appended atoms
        unsigned lo = 0, hi = nb;                                    // first record with i > a
        while (lo < hi) {
            const unsigned mid = lo + ((hi - lo) >> 1);
            if (((unsigned)B[2 * (size_t)mid] & 0xffffu) <= (unsigned)a) lo = mid + 1; else hi = mid;
        }
        const unsigned row = lo + off_b0[a], inner = nb + t_b0 + off_bin[a];
        for (unsigned k = 0; k < f.n_bonds; ++k) {
            const unsigned fb = fv.bonds[f.bond0 + k], p = fb & 0xffu, q = fb >> 8 & 0xffu, ty = fb >> 16 & 0xffu;
            const unsigned i = p == 0 ? (unsigned)a : first + p - 1, j = first + q - 1;
            bond(k < f.n_bonds0 ? row + k : inner + (k - f.n_bonds0), bond_word0(i, j, ty, ty), w2);
        }
    }

    // ---- the molecule's own bonds, each moved back by the attachment bonds of the rows in front of its own ----
    for (unsigned k = tid; k < nb; k += EX_THREADS) {
        const unsigned long long w0 = B[2 * (size_t)k], w1 = B[2 * (size_t)k + 1];
        bond(k + off_b0[(unsigned)w0 & (EX_MAX - 1)], w0, w1);
    }
}

}  // namespace

hipError_t expand_pack_enqueue(const SymbolTables* st_dev, const FragView& fv, const PackedTables& t, const TablesOut& o,
                               unsigned short* origin, unsigned* totals, hipStream_t s) {
    return count_scan_fill(expand_kernel<false>, expand_kernel<true>, t.n, EX_THREADS, o, totals, s, t, st_dev, fv, o, origin);
}

}  // namespace mnx
