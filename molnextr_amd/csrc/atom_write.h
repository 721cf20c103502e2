// atom_write.h — what a writer puts down for one atom and the class it writes a bond record as, for everything that keys on those
// bytes (internal): the SMILES writer and the canonical ranks (smiles.hip), whose initial key is an atom's written bytes, and the
// path fingerprint (fingerprint.hip), whose atom key is a hash of the same bytes. One definition, so the three cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>

#include "atom_symbol.h"

namespace mnx {

constexpr unsigned B_SINGLE = 0, B_DOUBLE = 1, B_TRIPLE = 2, B_AROMATIC = 3, B_ANY = 4;

// the written class of a bond record's `type`: a wedge is a single bond
__device__ __forceinline__ unsigned bond_class(unsigned ty) {
    return (ty == 1 || ty == 5 || ty == 6) ? B_SINGLE : ty == 2 ? B_DOUBLE : ty == 3 ? B_TRIPLE : ty == 4 ? B_AROMATIC : B_ANY;
}

template <typename Put>
__device__ __forceinline__ void put_number(unsigned v, Put put) {       // decimal, v <= 999
    if (v >= 100) put((char)('0' + v / 100));
    if (v >= 10) put((char)('0' + v / 10 % 10));
    put((char)('0' + v % 10));
}

// One atom's text from its interpretation (atom_symbol.h), the two bytes of its element and its stereo mark (0 none, 1 '@',
// 2 '@@': only a bracket atom ever has one).
template <typename Put>
__device__ __forceinline__ void put_atom(unsigned w, unsigned el, unsigned mark, Put put) {
    const unsigned cls = info_cls(w);
    if (cls == CLS_PSEUDO) { put('*'); return; }
    if (cls == CLS_RNUM) { put('['); put_number(info_num(w), put); put('*'); put(']'); return; }
    const char e0 = (char)(el & 255u), e1 = (char)(el >> 8 & 255u);
    const bool bracket = (w & 4u) != 0;
    if (bracket) {
        put('[');
        if (info_num(w)) put_number(info_num(w), put);
    }
    put(e0 == 'R' && e1 == ' ' ? '*' : info_aromatic(w) ? (char)(e0 + 32) : e0);
    if (e1 != ' ') put(e1);
    if (bracket) {
        if (mark >= 1) put('@');
        if (mark >= 2) put('@');
        const int h = info_h(w), q = info_charge(w);
        if (h >= 1) put('H');
        if (h >= 2) put((char)('0' + h));
        if (q != 0) {
            put(q > 0 ? '+' : '-');
            if (q > 1 || q < -1) put_number((unsigned)(q > 0 ? q : -q), put);
        }
        put(']');
    }
}

}  // namespace mnx
