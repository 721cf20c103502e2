// formula_host.cpp — the tokenizer and the structure search of mnx_formula_pack (molnextr_amd/csrc/formula_search.h) as a program
// on the host, so that the host compiler's sanitizers see the very text a lane of the kernel runs:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/formula_host.cpp -o formula_host
// stdin, words separated by white space: the number of names, then per name `name has_fragment` (0 / 1; the names in bytewise
// order, 1..16 bytes each); the number of cases, then per case `label start max_steps` (the label without enclosing brackets).
// stdout, one line per case: `status steps n_atoms` (status 0 a structure, 1 none, 2 step limit) and behind it, for every atom of
// a structure, ` symbol parent order h` — the element or [Name], the atom it hangs on and the order of that bond (0 0 for atom 0),
// its H count. Exit status 2 and a message on stderr for input that is no such description.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../molnextr_amd/csrc/formula_search.h"

static int fail(const char* what, long at) {
    std::fprintf(stderr, "formula_host: %s (entry %ld)\n", what, at);
    return 2;
}

int main() {
    long n_names;
    if (std::scanf("%ld", &n_names) != 1 || n_names < 0 || n_names > 512) return fail("no number of names in 0..512", -1);
    std::vector<unsigned char> len(n_names), name(16 * (size_t)n_names, 0);
    std::vector<int> frag(n_names);
    for (long i = 0; i < n_names; ++i) {
        char word[64];
        int has;
        if (std::scanf("%63s %d", word, &has) != 2 || std::strlen(word) > 16) return fail("no `name has_fragment`", i);
        len[i] = (unsigned char)std::strlen(word);
        std::memcpy(&name[16 * (size_t)i], word, len[i]);
        frag[i] = has ? 0 : -1;
        if (i > 0) {
            const std::string a((const char*)&name[16 * (size_t)(i - 1)], len[i - 1]), b(word);
            if (!(a < b)) return fail("the names are not in bytewise order", i);
        }
    }
    const formula::Names names{(int)n_names, len.data(), name.data(), frag.data()};
    long cases;
    if (std::scanf("%ld", &cases) != 1 || cases < 0) return fail("no number of cases", -1);
    for (long c = 0; c < cases; ++c) {
        char word[64];
        unsigned start, max_steps;
        if (std::scanf("%63s %u %u", word, &start, &max_steps) != 3) return fail("no `label start max_steps`", c);
        const size_t n = std::strlen(word);
        // exactly the slots the search may use, so that a step beyond them is a step beyond an allocation
        std::vector<unsigned short> item(formula::MAX_ITEMS), snap(formula::MAX_ITEMS);
        std::vector<unsigned> atom(formula::MAX_ATOMS);
        std::vector<unsigned char> label(word, word + n);
        unsigned n_atoms = 0, steps = 0;
        const unsigned status = formula::search(names, label.data(), (unsigned)n, start, max_steps, item.data(), snap.data(),
                                                atom.data(), 1, &n_atoms, &steps);
        std::printf("%u %u %u", status, steps, status == formula::OK ? n_atoms : 0u);
        for (unsigned k = 0; status == formula::OK && k < n_atoms; ++k) {
            const unsigned w = atom[k], what = formula::atom_what(w);
            if (what >= formula::GROUP0) {
                const unsigned g = what - formula::GROUP0;
                std::printf(" [%.*s]", (int)len[g], (const char*)&name[16 * (size_t)g]);
            } else {
                const unsigned e = formula::element_word(what);
                std::printf((e >> 8 & 255u) == ' ' ? " %c" : " %c%c", (char)(e & 255u), (char)(e >> 8 & 255u));
            }
            std::printf(" %u %u %u", k ? formula::atom_parent(w) : 0u, k ? formula::atom_order(w) : 0u, formula::atom_h(w));
        }
        std::printf("\n");
    }
    return 0;
}
