// kekule_host.cpp — the matching search of mnx_kekulize_pack (molnextr_amd/csrc/kekule_search.h) as a program on the host, so that
// the host compiler's sanitizers see the very text a lane of the kernel runs:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/kekule_host.cpp -o kekule_host
// stdin, numbers separated by white space: the number of cases; per case `n max_steps`, then per atom `system k v1 .. vk` —
// the system it is searched in (the system's lowest atom; 1023 for an atom that takes no part) and its k <= 3 needy neighbours in
// ascending order. stdout, per case: one line `system result steps` per system in ascending order (result 0 matched, 1 no
// matching, 2 step limit), then one line with every atom's partner (1023: none, and for every atom of a system that failed).
// Exit status 2 and a message on stderr for input that is no such description.
#include <cstdio>
#include <vector>

#include "../molnextr_amd/csrc/kekule_search.h"

static int fail(const char* what, long at) {
    std::fprintf(stderr, "kekule_host: %s (case %ld)\n", what, at);
    return 2;
}

int main() {
    long cases;
    if (std::scanf("%ld", &cases) != 1 || cases < 0) return fail("no number of cases", -1);
    for (long c = 0; c < cases; ++c) {
        unsigned n, max_steps;
        if (std::scanf("%u %u", &n, &max_steps) != 2) return fail("no `n max_steps`", c);
        if (n >= kekule::NONE) return fail("n beyond 1022", c);
        std::vector<unsigned> system(n), nbr(3 * (size_t)n, kekule::NONE), state(n, 0u), result(n, kekule::NONE);
        for (unsigned a = 0; a < n; ++a) {
            unsigned k;
            if (std::scanf("%u %u", &system[a], &k) != 2 || k > 3) return fail("no `system k` with k <= 3", c);
            if (system[a] != kekule::NONE && system[a] > a) return fail("a system is named by its lowest atom", c);
            for (unsigned q = 0; q < k; ++q)
                if (std::scanf("%u", &nbr[3 * (size_t)a + q]) != 1 || nbr[3 * (size_t)a + q] >= n) return fail("a neighbour is no atom", c);
        }
        for (unsigned a = 0; a < n; ++a)          // a neighbour list names needy atoms of the same system only
            for (unsigned q = 0; q < 3; ++q) {
                const unsigned v = nbr[3 * (size_t)a + q];
                if (v != kekule::NONE && (system[a] == kekule::NONE || system[v] != system[a] || v == a))
                    return fail("a neighbour outside the atom's system", c);
            }
        std::vector<bool> named(n, false);
        for (unsigned a = 0; a < n; ++a)
            if (system[a] != kekule::NONE) named[system[a]] = true;
        for (unsigned root = 0; root < n; ++root) {
            if (!named[root]) continue;
            unsigned steps = 0;
            result[root] = kekule::search(root, n, system.data(), nbr.data(), state.data(), max_steps, &steps);
            std::printf("%u %u %u\n", root, result[root], steps);
        }
        for (unsigned a = 0; a < n; ++a) {
            const bool matched = system[a] != kekule::NONE && result[system[a]] == kekule::OK;
            std::printf(a + 1 < n ? "%u " : "%u", matched ? kekule::partner(state[a]) : kekule::NONE);
        }
        std::printf("\n");
    }
    return 0;
}
