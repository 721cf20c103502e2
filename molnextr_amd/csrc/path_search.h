// path_search.h — the path walk of mnx_fingerprint_pack (fingerprint.hip), alone: one directed bond in, every path of 1 to
// max_bonds bonds that begins with it hashed and handed to the caller, their number out (the rule: include/molnextr_hip.h, "Path
// fingerprints"). Plain arrays and plain C++: no HIP, nothing of the engine, so that the same text runs in a lane of the kernel and
// in a program on the host (tools/paths_host.cpp), where the sanitizers of the host compiler see it. A call reads the lists and
// the keys and writes only its own stack, so calls for different bonds run side by side on the same arrays.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PATHS_HD __host__ __device__ __forceinline__
#else
#define PATHS_HD inline
#endif

namespace paths {

constexpr unsigned MAX_BONDS = 7;               // the longest path: 8 atoms, the levels of a stack
constexpr unsigned LEVELS = MAX_BONDS + 1;
constexpr unsigned FNV_BASIS = 2166136261u, FNV_PRIME = 16777619u;
constexpr unsigned FNV_UNPRIME = 899433627u;    // FNV_PRIME * FNV_UNPRIME == 1 mod 2^32: a step of the hash can be taken back
static_assert((unsigned)(FNV_PRIME * FNV_UNPRIME) == 1u, "the inverse of the FNV prime");

PATHS_HD unsigned fnv(unsigned h, unsigned w) { return (h ^ w) * FNV_PRIME; }
PATHS_HD unsigned unfnv(unsigned h, unsigned w) { return (h * FNV_UNPRIME) ^ w; }
PATHS_HD unsigned fmix32(unsigned h) {          // murmur3's finaliser
    h ^= h >> 16; h *= 0x85EBCA6Bu;
    h ^= h >> 13; h *= 0xC2B2AE35u;
    return h ^ h >> 16;
}
// the hash of a path from the hashes of its word sequence read from either end
PATHS_HD unsigned path_hash(unsigned forward, unsigned backward) { return fmix32(forward < backward ? forward : backward); }
// the path of no bonds: the atom alone
PATHS_HD unsigned atom_hash(unsigned key) { return path_hash(fnv(FNV_BASIS, key), fnv(FNV_BASIS, key)); }

// ---- an entry of a neighbour list, the one definition (mol_graph.h builds the lists): bits 0-9 the neighbour, bits 10-12 the bond
//      word (1 .. 5; the SMILES writer keeps the written class there), bits 13-22 the list's owner, a kernel's own from ENTRY_BITS ----
constexpr unsigned ENTRY_ATOM_BITS = 10, ENTRY_BITS = 2 * ENTRY_ATOM_BITS + 3;
PATHS_HD unsigned entry(unsigned nbr, unsigned word, unsigned owner) { return nbr | word << 10 | owner << 13; }
PATHS_HD unsigned entry_nbr(unsigned e) { return e & 1023u; }
PATHS_HD unsigned entry_word(unsigned e) { return e >> 10 & 7u; }
PATHS_HD unsigned entry_owner(unsigned e) { return e >> 13 & 1023u; }
// ---- a level of the stack: bits 0-9 the atom, bits 10-12 the word of the bond that led to it, bits 16-26 its list cursor ----
PATHS_HD unsigned level(unsigned atom, unsigned word, unsigned cursor) { return atom | word << 10 | cursor << 16; }
PATHS_HD unsigned level_atom(unsigned w) { return w & 1023u; }
PATHS_HD unsigned level_word(unsigned w) { return w >> 10 & 7u; }
PATHS_HD unsigned level_cursor(unsigned w) { return w >> 16; }

// Every path that begins with the directed bond lst[first] (owner -> neighbour), depth first without recursion. off[a] ..
// off[a + 1]: the list of atom a in lst (off values below 2048); key[a]: its atom key. stk[l * stride], l < LEVELS: this call's
// stack, no initial value needed. hit(p) receives the hash of every path in the order the walk finds them. Returns the number
// of paths, or max_steps + 1 as soon as there are more than max_steps, the walk then broken off. The forward hash grows and
// shrinks with the stack (a step of FNV-1a has an inverse), the backward hash is taken from the stack, 2 * MAX_BONDS + 1 words
// at the most.
template <typename Hit>
PATHS_HD unsigned walk(unsigned first, const unsigned* off, const unsigned* lst, const unsigned* key, unsigned* stk, unsigned stride,
                       unsigned max_bonds, unsigned max_steps, Hit hit) {
    const unsigned e0 = lst[first], a0 = entry_owner(e0);
    unsigned count = 0, d = 0, h = fnv(FNV_BASIS, key[a0]);
    stk[0] = level(a0, 0u, first);
    for (;;) {
        const unsigned w = stk[d * stride], a = level_atom(w), cur = level_cursor(w);
        // the root offers its one bond, a full path none, every other atom its list
        const bool spent = d == 0 ? cur != first : (d == max_bonds || cur == off[a + 1]);
        if (spent) {
            if (d == 0) return count;
            h = unfnv(unfnv(h, key[a]), level_word(w));
            --d;
            continue;
        }
        stk[d * stride] = w + (1u << 16);
        const unsigned e = lst[cur], n = entry_nbr(e), c = entry_word(e);
        bool held = false;
        for (unsigned l = 0; l <= d; ++l) held = held || level_atom(stk[l * stride]) == n;
        if (held) continue;                           // a walk never returns to an atom it holds
        if (++count > max_steps) return count;
        ++d;
        stk[d * stride] = level(n, c, off[n]);
        h = fnv(fnv(h, c), key[n]);
        unsigned back = FNV_BASIS;
        for (unsigned l = d; l > 0; --l) {
            const unsigned x = stk[l * stride];
            back = fnv(fnv(back, key[level_atom(x)]), level_word(x));
        }
        hit(path_hash(h, fnv(back, key[a0])));
    }
}

}  // namespace paths
