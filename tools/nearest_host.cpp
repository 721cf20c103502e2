// nearest_host.cpp — the selection of mnx_tanimoto_search (molnextr_amd/csrc/nearest_select.h) as a program on the host, so that
// the host compiler's sanitizers see the very text the kernels run:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/nearest_host.cpp -o nearest_host
// stdin, numbers separated by white space: the number of cases; per case `k n_lists`, then per list its number of candidates and
// per candidate `both either index`. Every list takes its candidates in with nearest::insert, as a workgroup of the scan does;
// the lists are then merged into the first with nearest::merge, as the merge kernel does. Each list is exactly k entries on the
// heap. stdout, per case one line: the k entries of the merged list as `both either index`, 4294967295 being no row.
// Exit status 2 and a message on stderr for input that is no such description.
#include <cstdio>
#include <vector>

#include "../molnextr_amd/csrc/nearest_select.h"

static int fail(const char* what, long at) {
    std::fprintf(stderr, "nearest_host: %s (case %ld)\n", what, at);
    return 2;
}

int main() {
    long cases;
    if (std::scanf("%ld", &cases) != 1 || cases < 0) return fail("no number of cases", -1);
    for (long c = 0; c < cases; ++c) {
        unsigned k, n_lists;
        if (std::scanf("%u %u", &k, &n_lists) != 2) return fail("no `k n_lists`", c);
        if (k < 1 || k > 64 || n_lists < 1 || n_lists > 65536) return fail("k outside 1 .. 64 or n_lists outside 1 .. 65536", c);
        std::vector<std::vector<nearest::entry>> lists(n_lists);
        for (unsigned w = 0; w < n_lists; ++w) {
            lists[w].assign(k, nearest::EMPTY);
            unsigned m;
            if (std::scanf("%u", &m) != 1) return fail("no number of candidates", c);
            for (unsigned j = 0; j < m; ++j) {
                unsigned both, either, index;
                if (std::scanf("%u %u %u", &both, &either, &index) != 3) return fail("no `both either index`", c);
                if (both > either || either > 2048 || index == nearest::NONE) return fail("both > either, either > 2048 or no index", c);
                const nearest::entry e = nearest::pack(both, either, index);
                if (nearest::entry_both(e) != both || nearest::entry_either(e) != either || nearest::entry_index(e) != index)
                    return fail("an entry does not unpack to what was packed", c);
                const unsigned pos = nearest::insert(lists[w].data(), k, e);
                if (pos > k || (pos < k && lists[w][pos] != e)) return fail("insert reports a position that does not hold the entry", c);
            }
        }
        for (unsigned w = 1; w < n_lists; ++w) nearest::merge(lists[0].data(), k, lists[w].data());
        for (unsigned j = 0; j < k; ++j) {
            const nearest::entry e = lists[0][j];
            std::printf("%s%u %u %u", j ? " " : "", nearest::entry_both(e), nearest::entry_either(e), nearest::entry_index(e));
        }
        std::printf("\n");
    }
    return 0;
}
