// atom_spell.h — an interpreted atom written out again, for the passes that respell atoms on the packed tables (normalize.hip and
// kekulize.hip, through respell_pass.h, which packs the bytes into registers), once (internal): the element as one number, the organic subset, the hydrogens a reader infers at an unbracketed
// upper-case atom, and the symbol byte by byte — unbracketed where a reader infers what the brackets would say, else a bracket atom
// as smiles.hip spells one.
#pragma once
#include <hip/hip_runtime.h>

namespace mnx {

// the element of an interpreted atom as one number: its two bytes (atom_symbol.h: capitalised, a blank behind one letter)
constexpr unsigned EL(char a, char b = ' ') { return (unsigned)(unsigned char)a | (unsigned)(unsigned char)b << 8; }
__device__ __forceinline__ bool is_organic(unsigned el) {
    return el == EL('B') || el == EL('C') || el == EL('N') || el == EL('O') || el == EL('P') || el == EL('S') || el == EL('F') ||
           el == EL('C', 'l') || el == EL('B', 'r') || el == EL('I');
}
// the hydrogens a reader infers at an unbracketed upper-case atom with bond order sum bo: v - bo for the smallest normal
// valence v >= bo, 0 when there is none
__device__ __forceinline__ unsigned implicit_h(unsigned el, unsigned bo) {
    unsigned v1, v2 = 0, v3 = 0;
    if (el == EL('B')) v1 = 3;
    else if (el == EL('C')) v1 = 4;
    else if (el == EL('N') || el == EL('P')) { v1 = 3; v2 = 5; }
    else if (el == EL('O')) v1 = 2;
    else if (el == EL('S')) { v1 = 2; v2 = 4; v3 = 6; }
    else v1 = 1;                          // F, Cl, Br, I
    return bo <= v1 ? v1 - bo : bo <= v2 ? v2 - bo : bo <= v3 ? v3 - bo : 0u;
}

// An interpreted atom's new symbol, byte by byte: unbracketed when a reader infers everything the brackets would say, else a
// bracket atom as smiles.hip spells one (isotope, element, 'H', 'Hk', sign and count; 12 bytes at most). inferred: the H count a
// reader takes for the unbracketed spelling. Returns whether it was written without brackets.
template <typename Put>
__device__ __forceinline__ bool spell_atom(unsigned el, bool aromatic, unsigned iso, unsigned h, int q, unsigned inferred, Put put) {
    const char e0 = (char)(el & 255u), e1 = (char)(el >> 8 & 255u);
    const bool plain = is_organic(el) && iso == 0 && q == 0 && h == inferred;
    if (!plain) {
        put('[');
        if (iso >= 100) put((char)('0' + iso / 100));
        if (iso >= 10) put((char)('0' + iso / 10 % 10));
        if (iso >= 1) put((char)('0' + iso % 10));
    }
    put(aromatic ? (char)(e0 + 32) : e0);
    if (e1 != ' ') put(e1);
    if (!plain) {
        if (h >= 1) put('H');
        if (h >= 2) put((char)('0' + h));
        if (q != 0) {
            const unsigned v = (unsigned)(q > 0 ? q : -q);
            put(q > 0 ? '+' : '-');
            if (v >= 10) put((char)('0' + v / 10));
            if (v >= 2) put((char)('0' + v % 10));
        }
        put(']');
    }
    return plain;
}

}  // namespace mnx
