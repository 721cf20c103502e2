// paths_host.cpp — the path walk of mnx_fingerprint_pack (molnextr_amd/csrc/path_search.h) as a program on the host, so that the
// host compiler's sanitizers see the very text a lane of the kernel runs:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/paths_host.cpp -o paths_host
// stdin, numbers separated by white space: the number of cases; per case `n_atoms n_bonds max_bonds max_steps`, then the atoms'
// keys, then per bond `i j word` (word 1 .. 5, no pair twice). stdout, per case one line: the largest number of paths from one
// directed bond (4294967295 past max_steps, every word then 0), the number of bits set, and the 64 words of the fingerprint.
// Exit status 2 and a message on stderr for input that is no such description.
#include <cstdio>
#include <vector>

#include "../molnextr_amd/csrc/path_search.h"

static int fail(const char* what, long at) {
    std::fprintf(stderr, "paths_host: %s (case %ld)\n", what, at);
    return 2;
}

int main() {
    long cases;
    if (std::scanf("%ld", &cases) != 1 || cases < 0) return fail("no number of cases", -1);
    for (long c = 0; c < cases; ++c) {
        unsigned n, nb, max_bonds, max_steps;
        if (std::scanf("%u %u %u %u", &n, &nb, &max_bonds, &max_steps) != 4) return fail("no `n_atoms n_bonds max_bonds max_steps`", c);
        if (n > 999 || nb > 999) return fail("more than 999 atoms or bonds", c);
        if (max_bonds < 1 || max_bonds > paths::MAX_BONDS || max_steps < 1) return fail("max_bonds outside 1 .. 7 or no steps", c);
        std::vector<unsigned> key(n), bi(nb), bj(nb), bw(nb), off(n + 1, 0u), fill(n, 0u), lst(2 * (size_t)nb);
        for (unsigned a = 0; a < n; ++a)
            if (std::scanf("%u", &key[a]) != 1) return fail("no key", c);
        for (unsigned k = 0; k < nb; ++k) {
            if (std::scanf("%u %u %u", &bi[k], &bj[k], &bw[k]) != 3) return fail("no `i j word`", c);
            if (bi[k] >= n || bj[k] >= n || bi[k] == bj[k] || bw[k] < 1 || bw[k] > 5) return fail("a bond to no atom, to itself or of no word", c);
            for (unsigned q = 0; q < k; ++q)
                if ((bi[q] == bi[k] && bj[q] == bj[k]) || (bi[q] == bj[k] && bj[q] == bi[k])) return fail("a pair twice", c);
            ++off[bi[k] + 1];
            ++off[bj[k] + 1];
        }
        for (unsigned a = 0; a < n; ++a) off[a + 1] += off[a];
        for (unsigned k = 0; k < nb; ++k) {
            lst[off[bi[k]] + fill[bi[k]]++] = paths::entry(bj[k], bw[k], bi[k]);
            lst[off[bj[k]] + fill[bj[k]]++] = paths::entry(bi[k], bw[k], bj[k]);
        }
        std::vector<unsigned> stk(paths::LEVELS), words(64, 0u);      // exactly the levels a walk may touch
        auto hit = [&](unsigned p) {
            const unsigned t0 = p & 2047u, t1 = p >> 11 & 2047u;
            words[t0 >> 5] |= 1u << (t0 & 31u);
            words[t1 >> 5] |= 1u << (t1 & 31u);
        };
        for (unsigned a = 0; a < n; ++a) hit(paths::atom_hash(key[a]));
        unsigned most = 0;
        for (unsigned s = 0; s < 2 * nb && most <= max_steps; ++s) {
            const unsigned p = paths::walk(s, off.data(), lst.data(), key.data(), stk.data(), 1u, max_bonds, max_steps, hit);
            most = p > most ? p : most;
        }
        const bool limited = most > max_steps;
        unsigned n_bits = 0;
        for (unsigned w = 0; w < 64; ++w) {
            if (limited) words[w] = 0u;
            n_bits += (unsigned)__builtin_popcount(words[w]);
        }
        std::printf("%u %u", limited ? 4294967295u : most, n_bits);
        for (unsigned w = 0; w < 64; ++w) std::printf(" %u", words[w]);
        std::printf("\n");
    }
    return 0;
}
