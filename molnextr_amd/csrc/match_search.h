// match_search.h — the search of mnx_substructure_match (match.hip), alone: the order in which a query's atoms are placed, and from
// one root atom of the target every embedding of the query that begins there, handed to the caller, the steps taken out (the
// rule: include/molnextr_hip.h, "Substructure search"). Plain arrays and plain C++: no HIP, nothing of the engine, so that the
// same text runs in a lane of the kernel and in a program on the host (tools/match_host.cpp), where the sanitizers of the host
// compiler see it. A search reads the query, the target's lists and match words and writes only its own stack, so searches from
// different roots run side by side on the same arrays.
#pragma once

#include "path_search.h"

namespace match {

using paths::entry_nbr, paths::entry_word, paths::level, paths::level_atom, paths::level_cursor;

constexpr unsigned MAX_QUERY = 64, MAX_QUERY_BONDS = 128;   // a query's atoms: the levels of a stack, the side of its bond matrix
constexpr unsigned NO_PARENT = 255;                         // parent[k] of the first atom of a component
constexpr unsigned ANY_BOND = 5;                            // the bond word (class + 1) of a query bond that matches every bond

// ---- an atom's match word: bits 0-4 the element's first letter - 'A', bits 5-9 its second letter - 'a' + 1 (0: none), bit 10
//      aromatic, bits 11-15 charge + 15, bits 16-25 isotope; bit 31 alone for an atom that is no plain atom — a pseudo-atom, a numbered
//      R-group, a '*': as a query atom it matches every atom, as a target atom only such a query atom ----
constexpr unsigned WORD_STAR = 1u << 31;
PATHS_HD unsigned atom_word(unsigned e0, unsigned e1, bool aromatic, int charge, unsigned isotope) {
    return (e0 - 'A') | (e1 == ' ' ? 0u : e1 - 'a' + 1u) << 5 | (aromatic ? 1u << 10 : 0u) | (unsigned)(charge + 15) << 11 | isotope << 16;
}
PATHS_HD bool atoms_match(unsigned q, unsigned t) {
    if (q & WORD_STAR) return true;
    if ((t & WORD_STAR) || ((q ^ t) & 0xFFFFu)) return false;
    const unsigned iso = q >> 16 & 1023u;
    return iso == 0 || iso == (t >> 16 & 1023u);
}
PATHS_HD bool bonds_match(unsigned q, unsigned t) { return t != 0 && (q == ANY_BOND || q == t); }

// The order: breadth first from the lowest atom not yet placed, an atom's neighbours in ascending index, until every atom is
// placed. adj[a * MAX_QUERY + b]: the bond word of the query bond a - b, 0 for none. order[k]: the atom at position k; parent[k]:
// the POSITION of its breadth-first parent, NO_PARENT for the first atom of a component. The queue is `order` itself.
PATHS_HD void build_order(unsigned nq, const unsigned char* adj, unsigned char* order, unsigned char* parent) {
    unsigned long long placed = 0;
    unsigned head = 0, tail = 0;
    for (unsigned first = 0; first < nq; ++first) {
        if (placed >> first & 1u) continue;
        placed |= 1ull << first;
        order[tail] = (unsigned char)first;
        parent[tail++] = (unsigned char)NO_PARENT;
        for (; head < tail; ++head) {
            const unsigned a = order[head];
            for (unsigned b = 0; b < nq; ++b) {
                if (!adj[a * MAX_QUERY + b] || (placed >> b & 1u)) continue;
                placed |= 1ull << b;
                order[tail] = (unsigned char)b;
                parent[tail++] = (unsigned char)head;
            }
        }
    }
}

// the bond word of the target bond a - b, 0 for none: a's list is sorted by neighbour
PATHS_HD unsigned bond_between(unsigned a, unsigned b, const unsigned* off, const unsigned* lst) {
    unsigned lo = off[a], hi = off[a + 1];
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1, n = entry_nbr(lst[mid]);
        if (n == b) return entry_word(lst[mid]);
        if (n < b) lo = mid + 1; else hi = mid;
    }
    return 0u;
}

// Every embedding whose first atom (position 0) lies on target atom `root`, depth first without recursion, in the lexicographic
// order of the image sequences. nq >= 1 query atoms in `order` with `parent`, qw[a] their match words, adj their bond words;
// nt target atoms, tw[t] their match words, off / lst their lists SORTED by neighbour (off values below 2048). stk[k * stride],
// k < nq: this call's stack, no initial value needed — level k holds the image of position k in bits 0-9 and the cursor of its
// candidates from bit 16: a slot of the list of the parent's image, or a target atom where the position has no parent.
// emit() is called at every embedding, the images then in the stack. Returns the steps S(root): 1 for the root and 1 for every
// candidate examined; max_steps + 1 as soon as there are more than max_steps, the search then broken off. *found: the
// embeddings, the search ended at the max_matches-th.
template <typename Emit>
PATHS_HD unsigned search(unsigned root, unsigned nq, const unsigned char* order, const unsigned char* parent, const unsigned* qw,
                         const unsigned char* adj, unsigned nt, const unsigned* off, const unsigned* lst, const unsigned* tw,
                         unsigned* stk, unsigned stride, unsigned max_matches, unsigned max_steps, unsigned* found, Emit emit) {
    unsigned steps = 1, d = 1;
    *found = 0;
    if (!atoms_match(qw[order[0]], tw[root])) return steps;
    stk[0] = level(root, 0u, 0u);
    if (nq == 1) { *found = 1; emit(); return steps; }
    stk[stride] = level(0u, 0u, parent[1] == NO_PARENT ? 0u : off[root]);
    for (;;) {
        const unsigned w = stk[d * stride], cur = level_cursor(w), p = parent[d];
        const unsigned end = p == NO_PARENT ? nt : off[level_atom(stk[p * stride]) + 1];
        if (cur == end) {                                 // out of candidates: back to the position in front
            if (--d == 0) return steps;                   // the root is its position's one candidate
            continue;
        }
        if (++steps > max_steps) return steps;
        stk[d * stride] = w + (1u << 16);
        const unsigned cand = p == NO_PARENT ? cur : entry_nbr(lst[cur]), a = order[d];
        bool ok = atoms_match(qw[a], tw[cand]);
        for (unsigned l = 0; l < d && ok; ++l) ok = level_atom(stk[l * stride]) != cand;       // not yet an image
        for (unsigned l = 0; l < d && ok; ++l) {          // every query bond to an atom placed earlier lies on a matching bond
            const unsigned q = adj[a * MAX_QUERY + order[l]];
            if (q) ok = bonds_match(q, bond_between(cand, level_atom(stk[l * stride]), off, lst));
        }
        if (!ok) continue;
        stk[d * stride] = level(cand, 0u, cur + 1u);
        if (d + 1 == nq) {
            emit();
            if (++*found == max_matches) return steps;
            continue;
        }
        ++d;
        stk[d * stride] = level(0u, 0u, parent[d] == NO_PARENT ? 0u : off[level_atom(stk[parent[d] * stride])]);
    }
}

}  // namespace match
