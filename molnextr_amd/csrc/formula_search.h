// formula_search.h — the tokenizer and the structure search of mnx_formula_pack (formula.hip), alone: one condensed-formula label
// in, its atoms and bonds out (the rule: include/molnextr_hip.h, "Tokens", "Units", "The search"). Plain arrays and plain C++: no
// HIP, nothing of the engine, so that the same text runs in a lane of the kernel and in a program on the host
// (tools/formula_host.cpp), where the sanitizers of the host compiler see it. No recursion: the units of the label lie flat in
// `item`, a parenthesis knows its partner, and the state in front of every item is kept in `snap`, so that backtracking is a step
// back in two arrays. Every array is read and written at [slot * stride]: a lane of the kernel keeps its slots `stride` lanes
// apart in LDS, the host program passes stride 1.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FORMULA_HD __host__ __device__ __forceinline__
#else
#define FORMULA_HD inline
#endif

namespace formula {

constexpr unsigned OK = 0, NO_STRUCTURE = 1, LIMIT = 2;      // NO_STRUCTURE: no tokenisation, no structure, or too large
constexpr unsigned MAX_LABEL = 20, MIN_LABEL = 2, MAX_ATOMS = 32, MAX_ITEMS = 96, MAX_DEPTH = 3, MAX_COUNT = 99;
constexpr unsigned DEFAULT_STEPS = 4096;
constexpr unsigned N_ELEMENTS = 12;       // index 0 is H
constexpr unsigned GROUP0 = 16;           // an atom's `what`: below N_ELEMENTS an element, GROUP0 + i the name i of the tables

// ---- the valence table: element e0 e1 (a blank behind one letter), its valences in the order of trial, 0 behind them ----
FORMULA_HD unsigned element_word(unsigned e) {      // e0 | e1 << 8 | valences, 4 bits each from bit 16
    switch (e) {
        case 0: return 'H' | ' ' << 8 | 0x001u << 16;
        case 1: return 'B' | ' ' << 8 | 0x003u << 16;
        case 2: return 'C' | ' ' << 8 | 0x004u << 16;
        case 3: return 'N' | ' ' << 8 | 0x053u << 16;
        case 4: return 'O' | ' ' << 8 | 0x002u << 16;
        case 5: return 'F' | ' ' << 8 | 0x001u << 16;
        case 6: return 'C' | 'l' << 8 | 0x001u << 16;
        case 7: return 'B' | 'r' << 8 | 0x001u << 16;
        case 8: return 'I' | ' ' << 8 | 0x001u << 16;
        case 9: return 'S' | 'i' << 8 | 0x004u << 16;
        case 10: return 'P' | ' ' << 8 | 0x035u << 16;
        default: return 'S' | ' ' << 8 | 0x246u << 16;
    }
}
// valence number c of `what` (a group token has the one valence 1), 0: there is none
FORMULA_HD unsigned valence_of(unsigned what, unsigned c) {
    if (what >= GROUP0) return c == 0 ? 1u : 0u;
    return c < 3 ? (element_word(what) >> (16 + 4 * c) & 15u) : 0u;
}
FORMULA_HD int element_of(unsigned char a, unsigned char b) {
    for (unsigned e = 0; e < N_ELEMENTS; ++e)
        if ((element_word(e) & 0xffffu) == ((unsigned)a | (unsigned)b << 8)) return (int)e;
    return -1;
}

// the names a group token may be: the sorted name table of mnx_set_symbol_tables with the fragment of every name (-1: none)
struct Names {
    int n;
    const unsigned char* len;        // [n] bytes of name i, 1..16
    const unsigned char* name;       // [n][16]
    const int* frag_of_name;         // [n]
};
FORMULA_HD int name_find(const Names& t, const unsigned char* s, int n) {
    int lo = 0, hi = t.n - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1, ml = t.len[mid];
        int c = 0;
        for (int k = 0; k < (n < ml ? n : ml) && c == 0; ++k) c = (int)s[k] - (int)t.name[16 * mid + k];
        if (c == 0) c = n - ml;
        if (c == 0) return mid;
        if (c < 0) hi = mid - 1; else lo = mid + 1;
    }
    return -1;
}
// the longest name with a fragment that begins at s (n bytes are left), its length in *len; -1: none
FORMULA_HD int longest_group(const Names& t, const unsigned char* s, int n, int* len) {
    for (int l = n < 16 ? n : 16; l >= 1; --l) {
        const int i = name_find(t, s, l);
        if (i >= 0 && t.frag_of_name[i] >= 0) { *len = l; return i; }
    }
    return -1;
}

// ---- an item, 16 bits: bits 0-1 kind, bits 2-3 the valence it tries, bits 4-15 arg — an ELEM's `what`, the count of an H item,
//      the partner of a parenthesis ----
constexpr unsigned ELEM = 0, HYD = 1, OPEN = 2, CLOSE = 3;
FORMULA_HD unsigned item_kind(unsigned w) { return w & 3u; }
FORMULA_HD unsigned item_choice(unsigned w) { return w >> 2 & 3u; }
FORMULA_HD unsigned item_arg(unsigned w) { return w >> 4; }
FORMULA_HD unsigned make_item(unsigned kind, unsigned arg) { return kind | arg << 4; }

// ---- the state in front of an item, 15 bits: bits 0-4 the current atom (with `pending`: the atom the next one hangs on), bit 5
//      pending — no current atom: the label or a branch begins —, bits 6-8 the current atom's free bonds, bits 9-14 atoms so far ----
FORMULA_HD unsigned st_cur(unsigned s) { return s & 31u; }
FORMULA_HD bool st_pending(unsigned s) { return (s >> 5 & 1u) != 0; }
FORMULA_HD unsigned st_free(unsigned s) { return s >> 6 & 7u; }
FORMULA_HD unsigned st_atoms(unsigned s) { return s >> 9 & 63u; }
FORMULA_HD unsigned make_state(unsigned cur, bool pending, unsigned free, unsigned atoms) {
    return cur | (pending ? 32u : 0u) | free << 6 | atoms << 9;
}

// ---- an atom of the structure: bits 0-9 what, bits 10-14 the atom it hangs on, bits 15-16 the order of that bond (atom 0:
//      neither), bits 17-19 its H count ----
FORMULA_HD unsigned atom_what(unsigned w) { return w & 1023u; }
FORMULA_HD unsigned atom_parent(unsigned w) { return w >> 10 & 31u; }
FORMULA_HD unsigned atom_order(unsigned w) { return w >> 15 & 3u; }
FORMULA_HD unsigned atom_h(unsigned w) { return w >> 17 & 7u; }

// The label's n bytes (brackets stripped) as flat items: counts are written out, `C` with a count n > 1 in front of an element
// with count m becomes n times C with m / n of it, the remainder behind the last. Returns the number of items, 0: the label
// stays (a byte outside the grammar, a count outside 1..99 or in no unit's place, depth beyond MAX_DEPTH, an empty
// parenthesis, more than MAX_ITEMS items or MAX_ATOMS heavy atoms and group tokens).
FORMULA_HD unsigned flatten(const Names& names, const unsigned char* s, unsigned n, unsigned short* item, unsigned stride) {
    unsigned out = 0, heavy = 0, depth = 0, open0 = 0, open1 = 0, open2 = 0;      // no array: a lane indexes none by a variable
    unsigned p = 0;
    auto digits = [&](unsigned* count) {          // a count behind a unit: 1 without digits; false: outside 1..99
        if (p >= n || s[p] < '0' || s[p] > '9') { *count = 1; return true; }
        unsigned v = 0;
        while (p < n && s[p] >= '0' && s[p] <= '9') { v = v * 10 + (unsigned)(s[p] - '0'); if (v > MAX_COUNT) return false; ++p; }
        *count = v;
        return v >= 1;
    };
    auto element_at = [&](unsigned at, unsigned* len) {     // the element of the maximal run [A-Z][a-z]* at `at`, -1: none
        if (at >= n || s[at] < 'A' || s[at] > 'Z') return -1;
        unsigned e = at + 1;
        while (e < n && s[e] >= 'a' && s[e] <= 'z') ++e;
        *len = e - at;
        return e - at == 1 ? element_of(s[at], ' ') : e - at == 2 ? element_of(s[at], s[at + 1]) : -1;
    };
    auto put = [&](unsigned kind, unsigned arg) {
        if (out >= MAX_ITEMS) { out = MAX_ITEMS + 1; return; }
        item[out * stride] = (unsigned short)make_item(kind, arg);
        ++out;
    };
    auto put_unit = [&](unsigned what, unsigned count) {    // count times an element or a group token; H as one item
        if (what == 0) { put(HYD, count); return; }
        for (unsigned k = 0; k < count; ++k) put(ELEM, what);
        heavy += count;
    };
    while (p < n) {
        if (out > MAX_ITEMS || heavy > MAX_ATOMS) return 0;
        const unsigned char c = s[p];
        if (c == '(') {
            if (depth >= MAX_DEPTH) return 0;
            if (depth == 0) open0 = out; else if (depth == 1) open1 = out; else open2 = out;
            ++depth;
            put(OPEN, 0);
            ++p;
            continue;
        }
        if (c == ')') {
            if (depth == 0) return 0;
            --depth;
            const unsigned from = depth == 0 ? open0 : depth == 1 ? open1 : open2;
            if (out > MAX_ITEMS || out == from + 1) return 0;                      // an empty parenthesis
            put(CLOSE, 0);
            ++p;
            unsigned count;
            if (!digits(&count)) return 0;
            const unsigned len = out - from;
            if (out > MAX_ITEMS || (unsigned long)len * count > MAX_ITEMS) return 0;
            for (unsigned k = 1; k < count; ++k)
                for (unsigned q = 0; q < len; ++q) {
                    const unsigned w = item[(from + q) * stride];
                    if (item_kind(w) == ELEM) ++heavy;
                    put(item_kind(w), item_arg(w));
                }
            continue;
        }
        unsigned len = 0, what;
        const int el = element_at(p, &len);
        if (el >= 0) { what = (unsigned)el; p += len; }
        else if ((c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z')) {
            int gl = 0;
            const int g = longest_group(names, s + p, (int)(n - p), &gl);
            if (g < 0) return 0;
            what = GROUP0 + (unsigned)g;
            p += (unsigned)gl;
        } else return 0;
        unsigned count;
        if (!digits(&count)) return 0;
        unsigned xl = 0;
        const int x = what == 2 && count > 1 ? element_at(p, &xl) : -1;           // C with a count in front of an element
        if (x >= 0) {
            p += xl;
            unsigned m;
            if (!digits(&m)) return 0;
            for (unsigned k = 0; k < count; ++k) {
                put_unit(2, 1);
                if (m / count) put_unit((unsigned)x, m / count);
            }
            if (m % count) put_unit((unsigned)x, m % count);
        } else put_unit(what, count);
    }
    if (depth != 0 || out > MAX_ITEMS || heavy > MAX_ATOMS || heavy == 0) return 0;
    return out;
}

// the items in the other direction, and every parenthesis' partner into its arg
FORMULA_HD void reverse_items(unsigned short* item, unsigned stride, unsigned n_items) {
    for (unsigned a = 0, b = n_items - 1; a < b; ++a, --b) {
        const unsigned short t = item[a * stride];
        item[a * stride] = item[b * stride];
        item[b * stride] = t;
    }
    for (unsigned p = 0; p < n_items; ++p) {
        const unsigned w = item[p * stride];
        if (item_kind(w) >= OPEN) item[p * stride] = (unsigned short)make_item(item_kind(w) ^ 1u, 0);
    }
}
FORMULA_HD void pair_parentheses(unsigned short* item, unsigned stride, unsigned n_items) {
    unsigned open0 = 0, open1 = 0, open2 = 0, depth = 0;
    for (unsigned p = 0; p < n_items; ++p) {
        const unsigned k = item_kind(item[p * stride]);
        if (k == OPEN) {
            if (depth == 0) open0 = p; else if (depth == 1) open1 = p; else open2 = p;
            ++depth;
        } else if (k == CLOSE) {
            --depth;
            const unsigned from = depth == 0 ? open0 : depth == 1 ? open1 : open2;
            item[p * stride] = (unsigned short)make_item(CLOSE, from);
            item[from * stride] = (unsigned short)make_item(OPEN, p);
        }
    }
}

// One direction: the items placed in order with the label's `start` bonds on the first atom; valences in table order with
// backtracking; *steps counts the placements of this label and is checked against max_steps. Behind OK atom[k * stride] holds
// atom k of *n_atoms (H counts and the raised orders of branches included).
FORMULA_HD unsigned search_items(unsigned short* item, unsigned short* snap, unsigned* atom, unsigned stride, unsigned n_items,
                                 unsigned start, unsigned max_steps, unsigned* steps, unsigned* n_atoms) {
    for (unsigned p = 0; p < n_items; ++p) item[p * stride] &= (unsigned short)~12u;
    unsigned p = 0, state = make_state(0, true, 0, 0);
    for (;;) {
        bool ok;
        if (p == n_items) {
            if (!st_pending(state) && st_free(state) == 0) break;
            ok = false;
        } else {
            snap[p * stride] = (unsigned short)state;
            const unsigned w = item[p * stride], kind = item_kind(w), arg = item_arg(w);
            const unsigned cur = st_cur(state), free = st_free(state), na = st_atoms(state);
            const bool pending = st_pending(state);
            if (kind == ELEM) {
                if (++*steps > max_steps) return LIMIT;
                const unsigned v = valence_of(arg, item_choice(w));
                if (pending) {
                    const unsigned begin = na == 0 ? start : 1u;
                    ok = v >= begin;
                    if (ok) {
                        atom[na * stride] = arg | (na == 0 ? 0u : cur << 10 | begin << 15);
                        state = make_state(na, false, v - begin, na + 1);
                    }
                } else if (free == 0) ok = false;
                else {
                    const bool leaf = free > v;
                    const unsigned order = leaf ? v : free;
                    ok = order <= 3;
                    if (ok) {
                        atom[na * stride] = arg | cur << 10 | order << 15;
                        state = leaf ? make_state(cur, false, free - v, na + 1) : make_state(na, false, v - free, na + 1);
                    }
                }
            } else if (kind == HYD) {
                if (++*steps > max_steps) return LIMIT;
                ok = !pending && free >= arg;
                if (ok) state = make_state(cur, false, free - arg, na);
            } else if (kind == OPEN) {
                ok = pending || free >= 1;
                if (ok && !pending && free > 1) state = make_state(cur, true, 0, na);          // a branch on cur
            } else {
                const unsigned outer = snap[arg * stride];
                ok = true;
                if (!st_pending(outer) && st_free(outer) > 1) {                                  // the branch ends
                    const unsigned order = 1 + free;
                    ok = !pending && order <= 3 && order <= st_free(outer);
                    if (ok) state = make_state(st_cur(outer), false, st_free(outer) - order, na);
                }
            }
        }
        if (ok) { ++p; continue; }
        // back to the last element that has another valence to try
        bool again = false;
        for (unsigned q = p == n_items ? p : p + 1; q-- > 0;) {
            const unsigned w = item[q * stride];
            if (item_kind(w) == ELEM && valence_of(item_arg(w), item_choice(w) + 1) != 0) {
                item[q * stride] = (unsigned short)(w + 4u);
                state = snap[q * stride];
                p = q;
                again = true;
                break;
            }
            item[q * stride] = (unsigned short)(w & ~12u);
        }
        if (!again) return NO_STRUCTURE;
    }
    // the hydrogens onto their atoms, and a branch's left-over bonds into the order of its joining bond
    for (unsigned q = 0; q < n_items; ++q) {
        const unsigned w = item[q * stride], s = snap[q * stride];
        if (item_kind(w) == HYD) atom[st_cur(s) * stride] += item_arg(w) << 17;
        else if (item_kind(w) == CLOSE) {
            const unsigned outer = snap[item_arg(w) * stride];
            if (!st_pending(outer) && st_free(outer) > 1) atom[st_atoms(outer) * stride] += st_free(s) << 15;
        }
    }
    *n_atoms = st_atoms(state);
    return OK;
}

// A label's n bytes (brackets stripped, MIN_LABEL..MAX_LABEL of them) with `start` bonds from the molecule: direction 1, then
// direction -1. max_steps 0: DEFAULT_STEPS. item and snap need MAX_ITEMS slots, atom MAX_ATOMS.
FORMULA_HD unsigned search(const Names& names, const unsigned char* s, unsigned n, unsigned start, unsigned max_steps,
                           unsigned short* item, unsigned short* snap, unsigned* atom, unsigned stride, unsigned* n_atoms,
                           unsigned* steps) {
    *steps = 0;
    *n_atoms = 0;
    if (n < MIN_LABEL || n > MAX_LABEL || start > 6) return NO_STRUCTURE;
    const unsigned n_items = flatten(names, s, n, item, stride);
    if (n_items == 0) return NO_STRUCTURE;
    const unsigned limit = max_steps ? max_steps : DEFAULT_STEPS;
    pair_parentheses(item, stride, n_items);
    unsigned r = search_items(item, snap, atom, stride, n_items, start, limit, steps, n_atoms);
    if (r != NO_STRUCTURE) return r;
    reverse_items(item, stride, n_items);
    pair_parentheses(item, stride, n_items);
    return search_items(item, snap, atom, stride, n_items, start, limit, steps, n_atoms);
}

// the bond order sum of atom k of a structure of n atoms (atom 0: with the label's `start` bonds), without its hydrogens
FORMULA_HD unsigned bond_sum(const unsigned* atom, unsigned stride, unsigned n, unsigned k, unsigned start) {
    unsigned sum = k == 0 ? start : atom_order(atom[k * stride]);
    for (unsigned c = k + 1; c < n; ++c)
        if (atom_parent(atom[c * stride]) == k) sum += atom_order(atom[c * stride]);
    return sum;
}

}  // namespace formula
