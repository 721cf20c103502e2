// respell_pass.h — the frame of a pass that respells atoms in place on the packed molecule tables (normalize.hip, kekulize.hip),
// once (internal): packed tables in, packed tables of the same record types out, atom and bond counts and order unchanged, every
// atom with a new or a copied symbol. One workgroup of RS_THREADS per molecule, run twice (count, fill; tables_out.h). A pass says
// which atoms it respells, how, and which bonds change their type; where the symbols go and what is written is here, who is
// admitted and what a refusal leaves is table_pass.h, shared with grow_pass.h. LDS atomics count, add up, hand out the slots of
// a list that is sorted afterwards, set bits of sets and take the minimum of a set: no atomic decides a position, an order or a
// result.
#pragma once
#include "atom_spell.h"
#include "table_pass.h"

namespace mnx {

constexpr int RS_THREADS = 256;
constexpr int RS_MAX = 1024;             // atoms and bond records held in LDS (999 at most)
constexpr int RS_PER = RS_MAX / RS_THREADS;
constexpr unsigned RS_NONE = 0xFFFFFFFFu;

// bits 0-3 of a pass's state word per atom and of its note: the H count
__device__ __forceinline__ unsigned st_h(unsigned s) { return s & MNX_NOTE_H_MASK; }

// ---- nbr3: the first three bonds (of some kind) of every atom, three words each, RS_NONE where there is none ----
// a bond record takes one slot at i and one at j, any slot: the three are sorted afterwards
__device__ __forceinline__ void hand_out_slots(unsigned* cnt, unsigned* nbr3, unsigned i, unsigned at_i, unsigned j, unsigned at_j) {
    const unsigned si = atomicAdd(&cnt[i], 1u), sj = atomicAdd(&cnt[j], 1u);
    if (si < 3) nbr3[3 * i + si] = at_i;
    if (sj < 3) nbr3[3 * j + sj] = at_j;
}
// an atom's three slots in ascending order, in LDS and in e0 <= e1 <= e2
__device__ __forceinline__ void sort_slots(unsigned* slots, unsigned& e0, unsigned& e1, unsigned& e2) {
    unsigned x;
    e0 = slots[0]; e1 = slots[1]; e2 = slots[2];
    if (e0 > e1) { x = e0; e0 = e1; e1 = x; }
    if (e1 > e2) { x = e1; e1 = e2; e2 = x; }
    if (e0 > e1) { x = e0; e0 = e1; e1 = x; }
    slots[0] = e0; slots[1] = e1; slots[2] = e2;
}

// ---- a symbol in registers: bytes 0-7 (the first in the low byte), bytes 8-11, and how many; of a copied symbol only len ----
struct Spelled { unsigned long long lo; unsigned hi, len; };
// spell_atom (atom_spell.h) into s; returns whether it was written without brackets
__device__ __forceinline__ bool spell_packed(Spelled& s, unsigned el, bool aromatic, unsigned iso, unsigned h, int q, unsigned inferred) {
    unsigned n = 0;
    unsigned long long lo = 0;
    unsigned hi = 0;
    const bool plain = spell_atom(el, aromatic, iso, h, q, inferred, [&](char c) {
        if (n < 8u) lo |= (unsigned long long)(unsigned char)c << (8u * n);
        else if (n < 12u) hi |= (unsigned)(unsigned char)c << (8u * (n - 8u));
        ++n;
    });
    s.lo = lo; s.hi = hi; s.len = n;
    return plain;
}
// put_text (tables_out.h) for a symbol in registers
__device__ __forceinline__ void put_spelled(const TablesOut& o, unsigned long long at, const Spelled& s) {
    for (unsigned c = 0; c < s.len; ++c)
        if (at + c < o.text_cap) o.text[at + c] = (char)(c < 8u ? s.lo >> (8u * c) : (unsigned long long)(s.hi >> (8u * (c - 8u))));
}

// Molecule blockIdx.x in one workgroup of a respelling pass, count (FILL = false) or fill (table_pass.h).
template <bool FILL>
struct RespellPass : TablePass<FILL> {
    using P = TablePass<FILL>;
    using P::t; using P::o; using P::mol; using P::mo; using P::na; using P::nb; using P::A; using P::B; using P::record;

    __device__ __forceinline__ RespellPass(const PackedTables& t, const TablesOut& o, unsigned refused) : P(t, o, refused) {}
    // too large: more than the 999 atoms or bonds of RS_MAX
    __device__ __forceinline__ bool admitted() { return P::admitted((mol.flags & PT_TOO_LARGE) != 0); }

    // Every atom's new symbol: RS_PER neighbouring atoms per thread, placed by a prefix scan over their lengths (scan: 2 *
    // RS_THREADS words of LDS). spell(a, sym, note) sets atom a's note and either spells it into sym or returns true: the symbol
    // is copied from the input. Count ends here with the molecule's record, flag0 / flag1 in it where an atom's note holds
    // note0 / note1. Fill writes the atom records, the notes and the text.
    template <typename Spell>
    __device__ __forceinline__ void atoms(unsigned* scan, unsigned char* __restrict__ notes, unsigned note0, unsigned flag0,
                                          unsigned note1, unsigned flag1, Spell spell) {
        const int tid = threadIdx.x;
        const unsigned char* text_in = P::text_in();
        Spelled sym[RS_PER];
        unsigned note[RS_PER], sum = 0, copied = 0;        // bit q: this thread's atom q keeps its symbol
        int vote0 = 0, vote1 = 0;
#pragma unroll
        for (int q = 0; q < RS_PER; ++q) {
            const int a = RS_PER * tid + q;
            sym[q].lo = 0; sym[q].hi = 0; sym[q].len = 0; note[q] = 0;
            if (a >= na) continue;
            if (spell(a, sym[q], note[q])) {
                copied |= 1u << q;
                sym[q].len = (unsigned)(A[3 * (size_t)a] >> 32) & 0xffffu;
            }
            sum += sym[q].len;
            vote0 |= (int)(note[q] & note0);
            vote1 |= (int)(note[q] & note1);
        }
        unsigned total;
        unsigned at = block_scan_excl<RS_THREADS>(sum, scan, &total);
        if (!FILL) {
            vote0 = __syncthreads_or(vote0);
            vote1 = __syncthreads_or(vote1);
            record((unsigned)na, (unsigned)nb, total, (vote0 ? flag0 : 0u) | (vote1 ? flag1 : 0u));
            return;
        }
#pragma unroll
        for (int q = 0; q < RS_PER; ++q) {
            const int a = RS_PER * tid + q;
            if (a >= na) continue;
            const unsigned long long w0 = A[3 * (size_t)a], w1 = A[3 * (size_t)a + 1], w2 = A[3 * (size_t)a + 2];
            const unsigned long long rec = (unsigned long long)mo.atom0 + (unsigned)a, to = (unsigned long long)mo.text0 + at;
            if (put_atom(o, rec, atom_word0(at, sym[q].len, 0u) | (w0 & ATOM_INDEX_BITS), w1 & ATOM_BINS_BITS, w2) && notes)
                notes[rec] = (unsigned char)note[q];
            if (copied >> q & 1u) put_text(o, to, text_in + (unsigned)w0, sym[q].len);
            else put_spelled(o, to, sym[q]);
            at += sym[q].len;
        }
    }

    // fill: every bond record as it is, but with type = rev = new_type(k, i) of record k with first atom i where that is not 0
    template <typename NewType>
    __device__ __forceinline__ void bonds(NewType new_type) const {
        for (int k = threadIdx.x; k < (int)nb; k += RS_THREADS) {
            unsigned long long w0 = B[2 * (size_t)k] & BOND_FIELD_BITS;
            const unsigned long long ty = new_type(k, (unsigned)w0 & 0xffffu);
            if (ty) w0 = (w0 & 0xffffffffull) | ty << 32 | ty << 40;
            put_bond(o, (unsigned long long)mo.bond0 + (unsigned)k, w0, B[2 * (size_t)k + 1]);
        }
    }
};

}  // namespace mnx
