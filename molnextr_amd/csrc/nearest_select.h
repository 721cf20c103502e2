// nearest_select.h — the selection of mnx_tanimoto_search (nearest.hip), alone: what a candidate is, which of two comes first, the
// insertion of one into a sorted list of k and the merge of two such lists (the rule: include/molnextr_hip.h, "Nearest rows").
// Plain integers and plain C++: no HIP, nothing of the engine, so that the same text runs in the kernels and in a program on the
// host (tools/nearest_host.cpp), where the sanitizers of the host compiler see it. The order is total — no two rows of a library
// share an index — so the first k of a set are the same whatever the order the set is fed in and however it is split into lists.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NEAREST_HD __host__ __device__ __forceinline__
#else
#define NEAREST_HD inline
#endif

namespace nearest {

// ---- a candidate: both (12 bits) | either (12 bits) | index (32 bits); both <= either <= 2048 ----
typedef unsigned long long entry;
constexpr unsigned NONE = 0xFFFFFFFFu;                      // MNX_NEAREST_NONE: no row
NEAREST_HD entry pack(unsigned both, unsigned either, unsigned index) { return (entry)both << 44 | (entry)either << 32 | index; }
NEAREST_HD unsigned entry_both(entry e) { return (unsigned)(e >> 44) & 4095u; }
NEAREST_HD unsigned entry_either(entry e) { return (unsigned)(e >> 32) & 4095u; }
NEAREST_HD unsigned entry_index(entry e) { return (unsigned)e; }
// the entry of an empty slot: it scores 0 / 1 and its index lies behind every row's, so every row comes before it
constexpr entry EMPTY = (entry)NONE;

// x comes before y: the larger fraction both / either (0 / 0 counting as 0 / 1), among equal fractions the lower index. The
// products stay below 2^23.
NEAREST_HD bool before(entry x, entry y) {
    const unsigned ex = entry_either(x), ey = entry_either(y);
    const unsigned px = entry_both(x) * (ey ? ey : 1u), py = entry_both(y) * (ex ? ex : 1u);
    return px > py || (px == py && entry_index(x) < entry_index(y));
}

// Slot i of a sorted list after candidate c went in at position pos (the number of entries that come before c): what slot i
// held (mine) in front of pos, c at pos, what slot i - 1 held (prev) behind it. A lane of a wave applies it to its own slot, the
// host loop below to every slot in turn: one rule.
NEAREST_HD entry slot_after(unsigned i, unsigned pos, entry mine, entry prev, entry c) { return i < pos ? mine : i == pos ? c : prev; }

// c into the sorted list of k entries, the last one dropped; returns its position, k when it comes behind all of them (then
// nothing changes)
NEAREST_HD unsigned insert(entry* list, unsigned k, entry c) {
    unsigned pos = 0;
    while (pos < k && before(list[pos], c)) ++pos;
    for (unsigned i = k; i-- > pos;) list[i] = slot_after(i, pos, list[i], i ? list[i - 1] : EMPTY, c);
    return pos;
}

// the sorted list `other` of k entries into the sorted list `list` of k entries: the first k of both. Once an entry of `other`
// comes behind the last of `list`, every later one does.
NEAREST_HD void merge(entry* list, unsigned k, const entry* other) {
    for (unsigned j = 0; j < k && before(other[j], list[k - 1]); ++j) insert(list, k, other[j]);
}

}  // namespace nearest
