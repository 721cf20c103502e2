// match_host.cpp — the search of mnx_substructure_match (molnextr_amd/csrc/match_search.h) as a program on the host, so that the
// host compiler's sanitizers see the very text a lane of the kernel runs:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/match_host.cpp -o match_host
// stdin, numbers separated by white space: the number of cases; per case `nq nq_bonds nt nt_bonds max_matches max_steps`, then the
// query's match words, per query bond `i j word`, the target's match words, per target bond `i j word` (word 1 .. 5, no pair twice
// on either side). stdout, per case one line: n_matches, steps, 1 when limited else 0, then the image of every query atom (65535
// without a match). A query without atoms gives `0 0 0`. Exit status 2 and a message on stderr for input that is no such description.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../molnextr_amd/csrc/match_search.h"

static int fail(const char* what, long at) {
    std::fprintf(stderr, "match_host: %s (case %ld)\n", what, at);
    return 2;
}

struct Side {
    unsigned n = 0, nb = 0;
    std::vector<unsigned> word, bi, bj, bw;
};

// 0, or what is wrong with the side
static const char* read_side(Side& s) {
    s.word.resize(s.n);
    s.bi.resize(s.nb); s.bj.resize(s.nb); s.bw.resize(s.nb);
    for (unsigned a = 0; a < s.n; ++a)
        if (std::scanf("%u", &s.word[a]) != 1) return "no match word";
    for (unsigned k = 0; k < s.nb; ++k) {
        if (std::scanf("%u %u %u", &s.bi[k], &s.bj[k], &s.bw[k]) != 3) return "no `i j word`";
        if (s.bi[k] >= s.n || s.bj[k] >= s.n || s.bi[k] == s.bj[k] || s.bw[k] < 1 || s.bw[k] > 5) return "a bond to no atom, to itself or of no word";
        for (unsigned q = 0; q < k; ++q)
            if ((s.bi[q] == s.bi[k] && s.bj[q] == s.bj[k]) || (s.bi[q] == s.bj[k] && s.bj[q] == s.bi[k])) return "a pair twice";
    }
    return nullptr;
}

int main() {
    long cases;
    if (std::scanf("%ld", &cases) != 1 || cases < 0) return fail("no number of cases", -1);
    for (long c = 0; c < cases; ++c) {
        Side q, t;
        unsigned max_matches, max_steps;
        if (std::scanf("%u %u %u %u %u %u", &q.n, &q.nb, &t.n, &t.nb, &max_matches, &max_steps) != 6)
            return fail("no `nq nq_bonds nt nt_bonds max_matches max_steps`", c);
        if (q.n > match::MAX_QUERY || q.nb > match::MAX_QUERY_BONDS) return fail("a query of more than 64 atoms or 128 bonds", c);
        if (t.n > 999 || t.nb > 999) return fail("a target of more than 999 atoms or bonds", c);
        if (max_matches < 1 || max_matches > 65535 || max_steps < 1 || max_steps > (1u << 20)) return fail("a limit outside its range", c);
        if (const char* why = read_side(q)) return fail(why, c);
        if (const char* why = read_side(t)) return fail(why, c);
        if (q.n == 0) { std::printf("0 0 0\n"); continue; }

        std::vector<unsigned char> adj(match::MAX_QUERY * match::MAX_QUERY, 0), order(q.n), parent(q.n);
        for (unsigned k = 0; k < q.nb; ++k)
            adj[q.bi[k] * match::MAX_QUERY + q.bj[k]] = adj[q.bj[k] * match::MAX_QUERY + q.bi[k]] = (unsigned char)q.bw[k];
        match::build_order(q.n, adj.data(), order.data(), parent.data());

        std::vector<unsigned> off(t.n + 1, 0u), fill(t.n, 0u), lst(2 * (size_t)t.nb);
        for (unsigned k = 0; k < t.nb; ++k) { ++off[t.bi[k] + 1]; ++off[t.bj[k] + 1]; }
        for (unsigned a = 0; a < t.n; ++a) off[a + 1] += off[a];
        for (unsigned k = 0; k < t.nb; ++k) {
            lst[off[t.bi[k]] + fill[t.bi[k]]++] = paths::entry(t.bj[k], t.bw[k], t.bi[k]);
            lst[off[t.bj[k]] + fill[t.bj[k]]++] = paths::entry(t.bi[k], t.bw[k], t.bj[k]);
        }
        for (unsigned a = 0; a < t.n; ++a)      // by neighbour: the low bits of an entry
            std::sort(lst.begin() + off[a], lst.begin() + off[a + 1], [](unsigned x, unsigned y) { return paths::entry_nbr(x) < paths::entry_nbr(y); });

        std::vector<unsigned> stk(q.n);         // exactly the levels a search may touch
        std::vector<unsigned> image(q.n, 65535u);
        unsigned long long total = 0;
        unsigned most = 0;
        bool broken = false, have = false;
        for (unsigned r = 0; r < t.n; ++r) {
            unsigned found = 0;
            const unsigned steps = match::search(r, q.n, order.data(), parent.data(), q.word.data(), adj.data(), t.n, off.data(), lst.data(),
                                                 t.word.data(), stk.data(), 1u, max_matches, max_steps, &found, [&] {
                if (have) return;
                have = true;
                for (unsigned k = 0; k < q.n; ++k) image[order[k]] = match::level_atom(stk[k]);
            });
            total += found;
            most = steps > most ? steps : most;
            broken = broken || steps > max_steps;
        }
        const unsigned n = total < max_matches ? (unsigned)total : max_matches;
        std::printf("%u %u %d", n, most, broken && n < max_matches ? 1 : 0);
        for (unsigned a = 0; a < q.n; ++a) std::printf(" %u", image[a]);
        std::printf("\n");
    }
    return 0;
}
