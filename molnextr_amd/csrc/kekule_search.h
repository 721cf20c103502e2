// kekule_search.h — the matching search of mnx_kekulize_pack (kekulize.hip), alone: one system of needy atoms in, the first perfect
// matching in the header's order out (the rule: include/molnextr_hip.h, "Matching"). Plain arrays and plain C++: no HIP, nothing of
// the engine, so that the same text runs in a lane of the kernel and in a program on the host (tools/kekule_host.cpp), where the
// sanitizers of the host compiler see it. One call works on one system and writes only the state words of that system's atoms, so
// calls for different systems may run side by side on the same arrays.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KEKULE_HD __host__ __device__ __forceinline__
#else
#define KEKULE_HD inline
#endif

namespace kekule {

constexpr unsigned NONE = 1023u;          // no atom: the molecules have 999 atoms at the most
constexpr unsigned OK = 0, NO_MATCHING = 1, LIMIT = 2;

// ---- an atom's state word: bits 0-9 its partner, bits 10-19 the next needy atom of its system, bits 20-29 the atom that chose
//      before it, bits 30-31 the slot it tries next ----
KEKULE_HD unsigned partner(unsigned w) { return w & 1023u; }
KEKULE_HD unsigned next_needy(unsigned w) { return w >> 10 & 1023u; }
KEKULE_HD unsigned chose_before(unsigned w) { return w >> 20 & 1023u; }
KEKULE_HD unsigned next_slot(unsigned w) { return w >> 30; }
KEKULE_HD unsigned with_partner(unsigned w, unsigned p) { return (w & ~1023u) | p; }
KEKULE_HD unsigned with_before(unsigned w, unsigned c) { return (w & ~(1023u << 20)) | c << 20; }
KEKULE_HD unsigned with_slot(unsigned w, unsigned q) { return (w & ~(3u << 30)) | q << 30; }

// whether the unmatched needy atom w has an unmatched needy neighbour left
KEKULE_HD bool has_free_neighbour(unsigned w, const unsigned* nbr, const unsigned* state) {
    bool any = false;
    for (unsigned q = 0; q < 3; ++q) {
        const unsigned x = nbr[3 * w + q];
        any = any || (x != NONE && partner(state[x]) == NONE);
    }
    return any;
}

// whether pairing the atom a has left one of a's needy neighbours unmatched and without an unmatched needy neighbour
KEKULE_HD bool strands_a_neighbour(unsigned a, const unsigned* nbr, const unsigned* state) {
    bool dead = false;
    for (unsigned q = 0; q < 3; ++q) {
        const unsigned w = nbr[3 * a + q];
        if (w != NONE && partner(state[w]) == NONE) dead = dead || !has_free_neighbour(w, nbr, state);
    }
    return dead;
}

// The system whose needy atoms are the a in root .. n - 1 with system[a] == root (root: the system's lowest atom, needy or not).
// nbr[3 * a + q]: the needy neighbours of the needy atom a in ascending order, NONE behind them. state[a] is written for the
// system's needy atoms only and needs no initial value; behind OK, partner(state[a]) is a's partner. *steps: the pairings tried,
// max_steps + 1 behind LIMIT. Depth first: the lowest unmatched atom tries its unmatched neighbours in ascending order, a pairing
// that strands a neighbour is undone at once, and an atom without a candidate left hands back to the atom that chose before it.
KEKULE_HD unsigned search(unsigned root, unsigned n, const unsigned* system, const unsigned* nbr, unsigned* state, unsigned max_steps,
                          unsigned* steps) {
    unsigned first = NONE, last = NONE, count = 0;
    bool lonely = false;
    for (unsigned a = root; a < n; ++a) {
        if (system[a] != root) continue;
        state[a] = NONE | NONE << 10 | NONE << 20;
        if (last == NONE) first = a;
        else state[last] = (state[last] & ~(1023u << 10)) | a << 10;
        last = a;
        ++count;
        lonely = lonely || nbr[3 * a] == NONE;
    }
    *steps = 0;
    if ((count & 1u) || lonely) return NO_MATCHING;
    if (count == 0) return OK;
    unsigned used = 0, cur = first;
    for (;;) {
        bool paired = false;
        while (next_slot(state[cur]) < 3) {
            const unsigned q = next_slot(state[cur]);
            state[cur] = with_slot(state[cur], q + 1);
            const unsigned v = nbr[3 * cur + q];
            if (v == NONE || partner(state[v]) != NONE) continue;
            if (++used > max_steps) { *steps = used; return LIMIT; }
            state[cur] = with_partner(state[cur], v);
            state[v] = with_partner(state[v], cur);
            if (strands_a_neighbour(cur, nbr, state) || strands_a_neighbour(v, nbr, state)) {
                state[cur] = with_partner(state[cur], NONE);
                state[v] = with_partner(state[v], NONE);
                continue;
            }
            paired = true;
            break;
        }
        if (paired) {
            unsigned nx = next_needy(state[cur]);
            while (nx != NONE && partner(state[nx]) != NONE) nx = next_needy(state[nx]);
            if (nx == NONE) break;        // every atom below cur was matched before cur chose: the matching is complete
            state[nx] = with_slot(with_before(state[nx], cur), 0);
            cur = nx;
        } else {
            const unsigned before = chose_before(state[cur]);
            if (before == NONE) { *steps = used; return NO_MATCHING; }
            cur = before;
            const unsigned v = partner(state[cur]);
            state[v] = with_partner(state[v], NONE);
            state[cur] = with_partner(state[cur], NONE);
        }
    }
    *steps = used;
    return OK;
}

}  // namespace kekule
