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
// bond records, which are sorted by i. That frame is grow_pass.h, shared with formula.hip; here is what a label is — an atom
// whose name has a fragment — and a fragment's atoms, symbols and bonds. The fragment tables are read from global memory (a few
// KB, shared by every workgroup of the launch).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/molnextr_hip.h"
#include "atom_symbol.h"
#include "grow_pass.h"
#include "table_passes.h"

namespace mnx {
namespace {

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
__global__ __launch_bounds__(GR_THREADS) void expand_kernel(
        const PackedTables t, const SymbolTables* __restrict__ st, const FragView fv, const TablesOut o,
        unsigned short* __restrict__ origin) {
    // fill: the five arrays of grow_pass.h; off_bin in 32 bits, a fragment of 32 atoms may hold 465 bonds among its appended atoms
    __shared__ unsigned off_atoms[FILL ? GR_MAX : 1], off_b0[FILL ? GR_MAX : 1], off_bin[FILL ? GR_MAX : 1];
    __shared__ unsigned off_text[FILL ? GR_MAX : 1], off_more[FILL ? GR_MAX : 1];
    __shared__ short frag_of[FILL ? GR_MAX : 1];
    __shared__ unsigned scan[2 * GR_THREADS];
    GrowPass<FILL, unsigned> p(t, o, MNX_MOL_EXPAND_REFUSED, origin, off_atoms, off_b0, off_bin, off_text, off_more);
    if (!p.admitted()) return;
    const int tid = threadIdx.x, na = p.na;

    // ---- every atom: GR_PER neighbouring atoms per thread ----
    int bad = 0, any = 0, left = 0;
    unsigned v[GR_SIZES][GR_PER];
#pragma unroll
    for (int q = 0; q < GR_PER; ++q) {
        const int a = GR_PER * tid + q;
        Grow g{-1, 0u, 0u, 0u, 0u, 0u, false};
        if (a < na) g = grow_of(t, st, fv, p.mol, a, &bad);
        if (FILL) frag_of[a] = (short)g.frag;
        any |= g.frag >= 0;
        left |= g.left;
        v[GR_ATOMS][q] = g.atoms; v[GR_B0][q] = g.bonds0; v[GR_BIN][q] = g.bonds_in; v[GR_TEXT][q] = g.text; v[GR_MORE][q] = g.text_more;
    }
    p.place(v, scan);
    if (!FILL) {
        const unsigned long long n_bonds = (unsigned long long)p.nb + p.total[GR_B0] + p.total[GR_BIN];
        if (p.bonds_refuse(bad || n_bonds > 0xffffffffull)) return;
        any = __syncthreads_or(any);
        left = __syncthreads_or(left);
        p.record((unsigned)na + p.total[GR_ATOMS], (unsigned)n_bonds, p.total[GR_TEXT] + p.total[GR_MORE],
                 (any ? MNX_MOL_EXPANDED : 0u) | (left ? MNX_MOL_LABEL_LEFT : 0u));
        return;
    }

    // ---- atoms and text: the molecule's own atoms keep their indices, a label's further atoms follow behind them ----
    for (int a = tid; a < na; a += GR_THREADS) {
        const int fi = frag_of[a];
        if (fi < 0) { p.put_own_atom(a); continue; }
        const unsigned long long w0 = p.A[3 * (size_t)a], w1 = p.A[3 * (size_t)a + 1], w2 = p.A[3 * (size_t)a + 2];
        const FragRec f = fv.frag[fi];
        const unsigned len0 = fv.atoms[f.atom0] >> 16;
        const unsigned first = p.first(a), more0 = p.more(a);
        for (unsigned q = 0; q < f.n_atoms; ++q) {
            const unsigned fa = fv.atoms[f.atom0 + q], fs0 = fa & 0xffffu, fl = fa >> 16;
            const unsigned at = q == 0 ? off_text[a] : more0 + fs0 - len0;
            p.put_record(q == 0 ? (unsigned)a : first + q - 1, at, fl, w0, w1, w2, (unsigned)a);
            put_text(o, (unsigned long long)p.mo.text0 + at, fv.text + f.text0 + fs0, fl);
        }
        // its bonds: those from the attachment atom behind the bond records of row a, the others in the rows of the appended atoms
        const unsigned row = p.row(a), inner = p.inner(a);
        for (unsigned k = 0; k < f.n_bonds; ++k) {
            const unsigned fb = fv.bonds[f.bond0 + k], i = fb & 0xffu, j = fb >> 8 & 0xffu, ty = fb >> 16 & 0xffu;
            p.put_new_bond(k < f.n_bonds0 ? row + k : inner + (k - f.n_bonds0), i == 0 ? (unsigned)a : first + i - 1, first + j - 1, ty, w2);
        }
    }
    p.own_bonds();
}

}  // namespace

hipError_t expand_pack_enqueue(const SymbolTables* st_dev, const FragView& fv, const PackedTables& t, const TablesOut& o,
                               unsigned short* origin, unsigned* totals, hipStream_t s) {
    return count_scan_fill(expand_kernel<false>, expand_kernel<true>, t.n, GR_THREADS, o, totals, s, t, st_dev, fv, o, origin);
}

}  // namespace mnx
