// formula.hip — condensed-formula labels replaced by the atoms and bonds they spell (mnx_formula_pack): what the reference's
// get_smiles_from_symbol does to an alias that is in neither of its tables, here by the project's own repaired rule (the rule
// stands in include/molnextr_hip.h; the tokenizer and the search are formula_search.h) and on the packed molecule tables — packed
// tables in, packed tables of the same record types out, in front of mnx_expand_pack, which expands the group tokens it leaves.
//   count  one workgroup per molecule: which atoms are candidate labels (atom_symbol.h reads the symbol, as the writers do), the
//          search of every candidate, the atoms / bonds / text bytes of the new molecule -> mols_out[b]
//   scan   exclusive scan of the three counts over the molecules -> atom0 / bond0 / text0, totals (tables_out.h)
//   fill   one workgroup per molecule: the searches again for the sizes, a prefix scan over the atoms, the molecule's own records,
//          and the searches a third time for the records of the labels
// One lane per candidate label runs the tokenizer and the search, FM_LANES labels at a time, each lane with its own slots of three
// LDS arrays (items, states, atoms), lane-minor, so that no lane indexes an array of its own by a variable. Every position follows
// from the prefix scan and, for a label's own row, from a binary search in the molecule's bond records, which are sorted by i: that
// frame is grow_pass.h, shared with expand.hip; here is what a label is and the atoms, symbols and bonds of the structure found.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/molnextr_hip.h"
#include "atom_spell.h"
#include "atom_symbol.h"
#include "formula_search.h"
#include "grow_pass.h"
#include "table_passes.h"

namespace mnx {
namespace {

constexpr int FM_LANES = 32;             // labels searched side by side: 16 KB of search state

static_assert(MNX_FORMULA_DEFAULT_STEPS == formula::DEFAULT_STEPS, "one default");

// what the search found for one label
struct Found {
    unsigned status;        // formula::OK, NO_STRUCTURE, LIMIT
    unsigned n, start;      // atoms of the structure; the label's bonds
};

// the element of a structure's atom as atom_spell.h numbers it
__device__ __forceinline__ unsigned el_of(unsigned what) { return formula::element_word(what) & 0xffffu; }

// the bytes of atom k of a label's structure, one by one to put: an element as atom_spell.h spells it, a group token as [Name]
template <typename Put>
__device__ __forceinline__ void spell_found(const SymbolTables* __restrict__ st, const unsigned* atom, const Found& f, unsigned k, Put put) {
    const unsigned w = atom[k * FM_LANES], what = formula::atom_what(w);
    if (what >= formula::GROUP0) {
        const unsigned name = what - formula::GROUP0;
        put('[');
        for (unsigned c = 0; c < st->len[name]; ++c) put((char)st->name[name][c]);
        put(']');
        return;
    }
    const unsigned el = el_of(what);
    spell_atom(el, false, 0u, formula::atom_h(w), 0, implicit_h(el, formula::bond_sum(atom, FM_LANES, f.n, k, f.start)), put);
}

template <bool FILL>
__global__ __launch_bounds__(GR_THREADS) void formula_kernel(
        const PackedTables t, const SymbolTables* __restrict__ st, const FragView fv, const TablesOut o,
        unsigned short* __restrict__ origin, const unsigned max_steps) {
    // fill: the five arrays of grow_pass.h, first the sizes, then their scan; a structure is a tree, 2047 x 31 bonds fit 16 bits
    __shared__ unsigned short off_atoms[FILL ? GR_MAX : 1], off_b0[FILL ? GR_MAX : 1], off_bin[FILL ? GR_MAX : 1];
    __shared__ unsigned off_text[FILL ? GR_MAX : 1], off_more[FILL ? GR_MAX : 1];
    __shared__ unsigned char replaced[FILL ? GR_MAX : 1];
    __shared__ unsigned short cand[GR_MAX];                       // the candidate labels in ascending order
    __shared__ unsigned short s_item[formula::MAX_ITEMS * FM_LANES], s_snap[formula::MAX_ITEMS * FM_LANES];
    __shared__ unsigned s_atom[formula::MAX_ATOMS * FM_LANES];
    __shared__ unsigned scan[2 * GR_THREADS];
    GrowPass<FILL, unsigned short> p(t, o, MNX_MOL_FORMULA_REFUSED, origin, off_atoms, off_b0, off_bin, off_text, off_more);
    if (!p.admitted()) return;
    const int tid = threadIdx.x, na = p.na;
    const unsigned nb = p.nb;
    const Molecule& mol = p.mol;
    const unsigned long long *A = p.A, *B = p.B;
    const unsigned char* text_in = p.text_in();

    // ---- every atom: GR_PER neighbouring atoms per thread; the candidates into their list ----
    int bad = 0;
    unsigned is_cand = 0, n_mine = 0;
#pragma unroll
    for (int q = 0; q < GR_PER; ++q) {
        const int a = GR_PER * tid + q;
        unsigned sl = 0;
        bool c = false;
        if (a < na) {
            const unsigned s0 = mol.A[a].sym0;
            sl = mol.A[a].sym_len;
            if ((unsigned long long)mol.m.text0 + s0 + sl > t.n_text_bytes) bad = 1;
            else {
                unsigned s3;
                int name;
                const unsigned char* s = text_in + s0;
                const unsigned w = interpret_atom(st, s, (int)sl, &s3, &name);
                const unsigned ni = sl >= 2 && s[0] == '[' && s[sl - 1] == ']' ? sl - 2 : sl;
                c = info_cls(w) == CLS_PSEUDO && name < 0 && ni >= formula::MIN_LABEL && ni <= formula::MAX_LABEL;
            }
        }
        if (FILL) { off_atoms[a] = 0; off_b0[a] = 0; off_bin[a] = 0; off_text[a] = sl; off_more[a] = 0; replaced[a] = 0; }
        if (c) { is_cand |= 1u << q; ++n_mine; }
    }
    if (!FILL && p.bonds_refuse(bad)) return;
    unsigned n_cand;
    {
        unsigned e = block_scan_excl<GR_THREADS>(n_mine, scan, &n_cand);
#pragma unroll
        for (int q = 0; q < GR_PER; ++q)
            if (is_cand >> q & 1u) cand[e++] = (unsigned short)(GR_PER * tid + q);
    }
    __syncthreads();

    const formula::Names names{st->n, st->len, &st->name[0][0], fv.frag_of_name};
    unsigned short* item = s_item + (tid & (FM_LANES - 1));
    unsigned short* snap = s_snap + (tid & (FM_LANES - 1));
    unsigned* atom = s_atom + (tid & (FM_LANES - 1));
    // the label at atom a: its bonds from the molecule (a class-4 bond or a type that is no bond order: the label stays), the search
    auto find = [&](unsigned a) {
        Found f{formula::NO_STRUCTURE, 0u, 0u};
        bool stays = false;
        for (unsigned k = 0; k < nb; ++k) {
            const unsigned long long w = B[2 * (size_t)k];
            if (((unsigned)w & 0xffffu) != a && ((unsigned)w >> 16) != a) continue;
            const unsigned ty = (unsigned)(w >> 32) & 0xffu;
            if (ty == 1 || ty == 5 || ty == 6) f.start += 1;
            else if (ty == 2 || ty == 3) f.start += ty;
            else stays = true;
            if (f.start > 7) f.start = 7;
        }
        if (stays) return f;
        const unsigned s0 = mol.A[a].sym0, sl = mol.A[a].sym_len;
        const unsigned char* s = text_in + s0;
        const bool strip = s[0] == '[' && s[sl - 1] == ']';
        unsigned steps;
        f.status = formula::search(names, strip ? s + 1 : s, strip ? sl - 2 : sl, f.start, max_steps, item, snap, atom, FM_LANES, &f.n, &steps);
        return f;
    };

    if (!FILL) {
        unsigned add_atoms = 0, add_text = 0, flags = 0;          // add_text: the difference, modulo 2^32
        for (unsigned base = 0; base < n_cand; base += FM_LANES) {
            if (tid >= FM_LANES || base + tid >= n_cand) continue;
            const unsigned a = cand[base + tid];
            const Found f = find(a);
            if (f.status != formula::OK) {
                flags |= MNX_MOL_FORMULA_LEFT | (f.status == formula::LIMIT ? MNX_MOL_FORMULA_LIMIT : 0u);
                continue;
            }
            flags |= MNX_MOL_FORMULA_EXPANDED;
            add_atoms += f.n - 1;
            unsigned bytes = 0;
            for (unsigned k = 0; k < f.n; ++k) spell_found(st, atom, f, k, [&](char) { ++bytes; });
            add_text += bytes - mol.A[a].sym_len;
        }
        unsigned own_text = 0, t_atoms, t_text, t_own;
#pragma unroll
        for (int q = 0; q < GR_PER; ++q)
            if (GR_PER * tid + q < na) own_text += mol.A[GR_PER * tid + q].sym_len;
        block_scan_excl<GR_THREADS>(add_atoms, scan, &t_atoms);
        block_scan_excl<GR_THREADS>(add_text, scan, &t_text);
        block_scan_excl<GR_THREADS>(own_text, scan, &t_own);
        const unsigned all = (__syncthreads_or((int)(flags & MNX_MOL_FORMULA_EXPANDED)) ? MNX_MOL_FORMULA_EXPANDED : 0u) |
                             (__syncthreads_or((int)(flags & MNX_MOL_FORMULA_LEFT)) ? MNX_MOL_FORMULA_LEFT : 0u) |
                             (__syncthreads_or((int)(flags & MNX_MOL_FORMULA_LIMIT)) ? MNX_MOL_FORMULA_LIMIT : 0u);
        const unsigned long long n_bonds = (unsigned long long)nb + t_atoms;
        if (n_bonds > 0xffffffffull) p.record(0, 0, 0, MNX_MOL_FORMULA_REFUSED);
        else p.record((unsigned)na + t_atoms, (unsigned)n_bonds, t_own + t_text, all);
        return;
    }

    // ---- fill, first the sizes of every label that is replaced ----
    for (unsigned base = 0; base < n_cand; base += FM_LANES) {
        if (tid >= FM_LANES || base + tid >= n_cand) continue;
        const unsigned a = cand[base + tid];
        const Found f = find(a);
        if (f.status != formula::OK) continue;
        unsigned b0 = 0, first = 0, more = 0;
        for (unsigned k = 1; k < f.n; ++k) b0 += formula::atom_parent(atom[k * FM_LANES]) == 0;
        spell_found(st, atom, f, 0, [&](char) { ++first; });
        for (unsigned k = 1; k < f.n; ++k) spell_found(st, atom, f, k, [&](char) { ++more; });
        off_atoms[a] = (unsigned short)(f.n - 1); off_b0[a] = (unsigned short)b0; off_bin[a] = (unsigned short)(f.n - 1 - b0);
        off_text[a] = first; off_more[a] = more; replaced[a] = 1;
    }
    __syncthreads();
    unsigned v[GR_SIZES][GR_PER];
#pragma unroll
    for (int q = 0; q < GR_PER; ++q) {
        const int a = GR_PER * tid + q;
        v[GR_ATOMS][q] = off_atoms[a]; v[GR_B0][q] = off_b0[a]; v[GR_BIN][q] = off_bin[a]; v[GR_TEXT][q] = off_text[a]; v[GR_MORE][q] = off_more[a];
    }
    p.place(v, scan);

    // ---- the molecule's own atoms and bonds ----
    for (int a = tid; a < na; a += GR_THREADS)
        if (!replaced[a]) p.put_own_atom(a);
    p.own_bonds();

    // ---- the labels: the first atom in the label's place, the others behind the molecule's own in placement order ----
    for (unsigned base = 0; base < n_cand; base += FM_LANES) {
        if (tid >= FM_LANES || base + tid >= n_cand) continue;
        const unsigned a = cand[base + tid];
        if (!replaced[a]) continue;
        const Found f = find(a);
        const unsigned long long w0 = A[3 * (size_t)a], w1 = A[3 * (size_t)a + 1], w2 = A[3 * (size_t)a + 2];
        const unsigned first = p.first(a);
        unsigned at = off_text[a];                                   // where the next symbol begins in the new text
        for (unsigned k = 0; k < f.n; ++k) {
            if (k == 1) at = p.more(a);
            unsigned len = 0;
            spell_found(st, atom, f, k, [&](char c) {
                const unsigned long long to = (unsigned long long)p.mo.text0 + at + len;
                if (to < o.text_cap) o.text[to] = c;
                ++len;
            });
            p.put_record(k == 0 ? a : first + k - 1, at, len, w0, w1, w2, a);
            at += len;
        }
        // its bonds: those from the first atom behind the bond records of row a, the others in the rows of the appended atoms
        const unsigned row = p.row(a), inner = p.inner(a);
        for (unsigned k = 1; k < f.n; ++k) {
            const unsigned w = atom[k * FM_LANES], pa = formula::atom_parent(w), ty = formula::atom_order(w);
            unsigned before = 0;                                     // the bonds in front of (pa, k) among those of its kind
            for (unsigned c = 1; c < f.n; ++c) {
                const unsigned pc = formula::atom_parent(atom[c * FM_LANES]);
                before += (pa == 0) ? (pc == 0 && c < k) : (pc != 0 && (pc < pa || (pc == pa && c < k)));
            }
            p.put_new_bond((pa == 0 ? row : inner) + before, pa == 0 ? a : first + pa - 1, first + k - 1, ty, w2);
        }
    }
}

}  // namespace

hipError_t formula_pack_enqueue(const SymbolTables* st_dev, const FragView& fv, const PackedTables& t, const TablesOut& o,
                                unsigned short* origin, unsigned* totals, unsigned max_steps, hipStream_t s) {
    return count_scan_fill(formula_kernel<false>, formula_kernel<true>, t.n, GR_THREADS, o, totals, s, t, st_dev, fv, o, origin, max_steps);
}

}  // namespace mnx
