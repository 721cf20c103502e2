// normalize.hip — one normal spelling per atom on the packed molecule tables (mnx_normalize_pack): aromatic rings perceived from
// Kekule drawings, hydrogens counted, brackets dropped where a reader infers what they say, so that every writer, the canonical
// ranks and mnx_expand_pack run on the result as they are. A pass of respell_pass.h, where its frame is: count, scan and fill,
// admission and refusal (table_pass.h), the slots, the symbols' placing, the records written. The rule stands in include/molnextr_hip.h: it is
// this library's own and not a toolkit's aromaticity model. Inside a workgroup, in count and again in fill: the atoms'
// interpretation (atom_symbol.h), then per atom its bond count, bond order sum and the first three of its bonds in LDS (a
// candidate atom has at most three, so a graph of any density costs one pass over its bond records and nothing that grows with a
// degree), then one thread per start atom walks the rings of 5 and 6 candidate atoms that begin at it — twice: once to mark the
// bonds and atoms that lie on such a ring, once to judge every ring —, then every atom's new symbol. Every loop has a bound known
// at compile time or is a stride over the molecule's records.
#include "respell_pass.h"
#include "table_passes.h"

namespace mnx {
namespace {

constexpr int NZ_WALK_STEPS = 384;      // 1 + 3 + 6 + 12 + 24 + 48 = 94 atoms on the walks from one start, four steps each

// ---- one of an atom's first three bonds: bits 0-9 the neighbour, bits 10-11 the order (1..3), bits 12-21 the bond record ----
__device__ __forceinline__ unsigned slot_nbr(unsigned e) { return e & 1023u; }
__device__ __forceinline__ unsigned slot_order(unsigned e) { return e >> 10 & 3u; }
__device__ __forceinline__ unsigned slot_bond(unsigned e) { return e >> 12 & 1023u; }

// ---- an atom's state word ----
//   bits 0-3 H count, bits 4-5 candidate kind (0 none, 1 (d), 2 (p), 3 (e)), bits 6-7 the slot of a (d) atom's double bond,
//   bit 8 copied uninterpreted, bit 9 excluded by one of its bonds (set by the bond loop), bits 10-12 slot q is a ring-system bond,
//   bit 13 the atom lies on an enumerated ring, bit 14 made aromatic, bits 15-17 slot q is a bond of an aromatic ring,
//   bit 18 the symbol is copied although the atom is interpreted (the four chiral carbons)
constexpr unsigned ST_KIND = 4, ST_DSLOT = 6, ST_COPY = 1u << 8, ST_EXCLUDED = 1u << 9, ST_RSB = 10, ST_ONRING = 1u << 13;
constexpr unsigned ST_AROMATIC = 1u << 14, ST_AB = 15, ST_KEEP = 1u << 18;
constexpr unsigned KIND_D = 1, KIND_P = 2, KIND_E = 3;
__device__ __forceinline__ unsigned st_kind(unsigned s) { return s >> ST_KIND & 3u; }
__device__ __forceinline__ unsigned st_dslot(unsigned s) { return s >> ST_DSLOT & 3u; }

// Every ring of 5 or 6 candidate atoms whose lowest atom is s, once: a depth-first walk from s over candidate neighbours of
// higher index, closed when it comes back to s behind 5 or 6 atoms; of a ring's two directions the one whose second atom lies
// below its last. The walk's atoms are 10-bit fields of `path` and the next slot to try at every depth a 2-bit field of `next`,
// so nothing is indexed in registers. found(path, n): the ring's n atoms are fields 0 .. n - 1 of path.
template <typename Found>
__device__ __forceinline__ void walk_rings(unsigned s, const unsigned* st, const unsigned* nbr3, Found found) {
    unsigned long long path = s;
    unsigned next = 0;
    int depth = 0;                        // the field of the walk's last atom
    for (int step = 0; step < NZ_WALK_STEPS; ++step) {
        const unsigned q = next >> (2 * depth) & 3u;
        if (q == 3u) {
            if (depth == 0) break;
            next &= ~(3u << (2 * depth));
            --depth;
            continue;
        }
        next += 1u << (2 * depth);
        const unsigned last = (unsigned)(path >> (10 * depth)) & 1023u;
        const unsigned e = nbr3[3 * last + q];
        if (e == RS_NONE) continue;
        const unsigned v = slot_nbr(e);
        if (v == s) {
            if (depth >= 4 && ((unsigned)(path >> 10) & 1023u) < last) found(path, depth + 1);
            continue;
        }
        if (v < s || depth == 5 || st_kind(st[v]) == 0) continue;
        bool seen = false;
#pragma unroll
        for (int d = 1; d < 6; ++d) seen |= d <= depth && ((unsigned)(path >> (10 * d)) & 1023u) == v;
        if (seen) continue;
        ++depth;
        path = (path & ~(1023ull << (10 * depth))) | (unsigned long long)v << (10 * depth);
    }
}

// the bit `base` + q of the slot q that holds atom u's bond to v (both candidates: u has at most three bonds, all to different
// atoms); 0 when there is none
__device__ __forceinline__ unsigned slot_bit(const unsigned* nbr3, unsigned u, unsigned v, unsigned base) {
    unsigned bit = 0;
#pragma unroll
    for (unsigned q = 0; q < 3; ++q) {
        const unsigned e = nbr3[3 * u + q];
        if (e != RS_NONE && slot_nbr(e) == v) bit = 1u << (base + q);
    }
    return bit;
}

template <bool FILL>
__global__ __launch_bounds__(RS_THREADS) void normalize_kernel(
        const PackedTables t, const SymbolTables* __restrict__ stab, const TablesOut o, unsigned char* __restrict__ notes) {
    __shared__ unsigned info[RS_MAX], elem[RS_MAX];
    __shared__ unsigned cnt[RS_MAX];      // bond records at the atom: hands out the slots of nbr3
    __shared__ unsigned acc[RS_MAX];      // bits 0-11 bond order sum, bits 12-21 double bonds, bits 22-31 triple bonds
    __shared__ unsigned st[RS_MAX];
    __shared__ unsigned nbr3[3 * RS_MAX];
    __shared__ unsigned scan[2 * RS_THREADS];
    const int tid = threadIdx.x;
    RespellPass<FILL> p(t, o, MNX_MOL_NORMALIZE_REFUSED);
    if (!p.admitted()) return;
    const int na = p.na, nb = p.nb;

    // ---- the atoms as the writers read them; per atom its bond count, order sum and first three bonds ----
    int bad = interpret_atoms<RS_MAX, RS_THREADS>(t, stab, p.mol, info, elem);
    for (int a = tid; a < RS_MAX; a += RS_THREADS) {
        cnt[a] = 0; acc[a] = 0; st[a] = 0;
        nbr3[3 * a] = nbr3[3 * a + 1] = nbr3[3 * a + 2] = RS_NONE;
    }
    __syncthreads();
    for (int k = tid; k < nb; k += RS_THREADS) {
        const auto [i, j, ty, beyond] = p.bond(k);
        if (beyond) { bad = 1; continue; }
        const unsigned order = (ty == 1 || ty == 5 || ty == 6) ? 1u : (ty == 2 || ty == 3) ? ty : 0u;
        if (order == 0 || i == j) {       // class 4, no class of a bond, or a bond from an atom to itself: both ends are copied
            atomicOr(&st[i], ST_EXCLUDED);
            atomicOr(&st[j], ST_EXCLUDED);
            continue;
        }
        const unsigned add = order | (order == 2 ? 1u << 12 : 0u) | (order == 3 ? 1u << 22 : 0u);
        hand_out_slots(cnt, nbr3, i, j | order << 10 | (unsigned)k << 12, j, i | order << 10 | (unsigned)k << 12);
        atomicAdd(&acc[i], add);          // sums and counts do not depend on the order of their terms
        atomicAdd(&acc[j], add);
    }
    if (p.refuses(bad)) return;           // a symbol beyond the text or a bond that is no bond of the molecule

    // ---- every atom: hydrogens, whether it is a candidate and of which kind; its three slots in ascending order ----
    for (int a = tid; a < na; a += RS_THREADS) {
        const unsigned w = info[a], el = elem[a] & 0xffffu, deg = cnt[a];
        const unsigned bo = acc[a] & 4095u, n_double = acc[a] >> 12 & 1023u, n_triple = acc[a] >> 22;
        unsigned e0, e1, e2;
        sort_slots(&nbr3[3 * a], e0, e1, e2);
        unsigned s = st[a] & ST_EXCLUDED;
        if (info_cls(w) != CLS_ATOM || info_aromatic(w) || el == EL('R') || s) {
            st[a] = s | ST_COPY | (info_cls(w) == CLS_ATOM ? (unsigned)info_h(w) : 0u);
            continue;
        }
        const bool bracket = (w & 4u) != 0, chiral = (w & 8u) != 0;
        const unsigned h = bracket ? (unsigned)info_h(w) : implicit_h(el, bo);
        const int q = info_charge(w);
        s = h | (chiral ? ST_KEEP : 0u);
        const bool c = el == EL('C'), n = el == EL('N'), os = el == EL('O') || el == EL('S');
        bool distinct = true;             // two bond records to one neighbour: no candidate
        if (deg >= 2) distinct = slot_nbr(e0) != slot_nbr(e1);
        if (deg == 3) distinct = distinct && slot_nbr(e1) != slot_nbr(e2) && slot_nbr(e0) != slot_nbr(e2);
        if ((c || n || os) && !chiral && deg <= 3 && n_triple == 0 && distinct) {
            if (n_double == 1 && ((c && q == 0) || (n && (q == 0 || q == 1)))) {
                const unsigned ds = slot_order(e0) == 2 ? 0u : slot_order(e1) == 2 ? 1u : 2u;
                s |= KIND_D << ST_KIND | ds << ST_DSLOT;
            } else if (n_double == 0 && ((n && q == 0 && deg + h == 3) || (os && q == 0 && deg == 2 && h == 0) ||
                                         (c && q == -1 && deg + h == 3))) {
                s |= KIND_P << ST_KIND;
            } else if (n_double == 0 && c && q == 1) {
                s |= KIND_E << ST_KIND;
            }
        }
        st[a] = s;
    }
    __syncthreads();

    // ---- the enumerated rings, first pass: which bonds are ring-system bonds, which atoms lie on an enumerated ring ----
    for (int a = tid; a < na; a += RS_THREADS) {
        if (st_kind(st[a]) == 0) continue;
        walk_rings((unsigned)a, st, nbr3, [&](unsigned long long path, int n) {
#pragma unroll
            for (int d = 0; d < 6; ++d) {
                if (d >= n) continue;
                const unsigned u = (unsigned)(path >> (10 * d)) & 1023u;
                const unsigned v = (unsigned)(path >> (10 * (d + 1 == n ? 0 : d + 1))) & 1023u;
                atomicOr(&st[u], ST_ONRING | slot_bit(nbr3, u, v, ST_RSB));
                atomicOr(&st[v], slot_bit(nbr3, v, u, ST_RSB));
            }
        });
    }
    __syncthreads();
    // ---- second pass: every ring's electrons; the atoms and bonds of a ring with 6 become aromatic. The verdict bits (14-17)
    //      are written here and read by no walk, so the verdicts do not depend on one another ----
    for (int a = tid; a < na; a += RS_THREADS) {
        if (st_kind(st[a]) == 0) continue;
        walk_rings((unsigned)a, st, nbr3, [&](unsigned long long path, int n) {
            unsigned electrons = 0;
            bool fails = false;
#pragma unroll
            for (int d = 0; d < 6; ++d) {
                if (d >= n) continue;
                const unsigned u = (unsigned)(path >> (10 * d)) & 1023u, su = st[u], kind = st_kind(su);
                if (kind == KIND_P) electrons += 2;
                else if (kind == KIND_D) {
                    const unsigned ds = st_dslot(su);
                    if (su >> (ST_RSB + ds) & 1u) electrons += 1;
                    else {
                        const unsigned x = slot_nbr(nbr3[3 * u + ds]), ex = elem[x] & 0xffffu;
                        const bool hetero = info_cls(info[x]) == CLS_ATOM && (ex == EL('O') || ex == EL('N') || ex == EL('S'));
                        if (!((elem[u] & 0xffffu) == EL('C') && hetero && !(st[x] & ST_ONRING))) fails = true;
                    }
                }
            }
            if (fails || electrons != 6) return;
#pragma unroll
            for (int d = 0; d < 6; ++d) {
                if (d >= n) continue;
                const unsigned u = (unsigned)(path >> (10 * d)) & 1023u;
                const unsigned v = (unsigned)(path >> (10 * (d + 1 == n ? 0 : d + 1))) & 1023u;
                atomicOr(&st[u], ST_AROMATIC | slot_bit(nbr3, u, v, ST_AB));
                atomicOr(&st[v], slot_bit(nbr3, v, u, ST_AB));
            }
        });
    }
    __syncthreads();

    // ---- every atom's new symbol; an atom copied uninterpreted and a chiral carbon keep theirs ----
    p.atoms(scan, notes, MNX_NOTE_AROMATIZED, MNX_MOL_AROMATIZED, MNX_NOTE_UNBRACKETED, MNX_MOL_UNBRACKETED,
            [&](int a, Spelled& sym, unsigned& note) {
                const unsigned s = st[a], w = info[a];
                note = st_h(s);
                if (s & ST_COPY) note |= MNX_NOTE_COPIED;
                if (s & (ST_COPY | ST_KEEP)) return true;
                const unsigned el = elem[a] & 0xffffu, deg = cnt[a], bo = acc[a] & 4095u;
                const bool aromatic = (s & ST_AROMATIC) != 0;
                const unsigned inferred = !aromatic ? implicit_h(el, bo) : el == EL('C') ? (deg <= 3 ? 3 - deg : 0u) : 0u;
                const bool plain = spell_packed(sym, el, aromatic, info_num(w), st_h(s), info_charge(w), inferred);
                if (aromatic) note |= MNX_NOTE_AROMATIZED;
                if (plain && (w & 4u)) note |= MNX_NOTE_UNBRACKETED;
                return false;
            });
    if (!FILL) return;
    // ---- the bonds: type = rev = 4 on an aromatic ring, every other record as it is ----
    p.bonds([&](int k, unsigned i) {
        const unsigned si = st[i];
        bool aromatic = false;
#pragma unroll
        for (unsigned q = 0; q < 3; ++q) {
            const unsigned e = nbr3[3 * i + q];
            aromatic |= e != RS_NONE && slot_bond(e) == (unsigned)k && (si >> (ST_AB + q) & 1u);
        }
        return aromatic ? 4ull : 0ull;
    });
}

}  // namespace

hipError_t normalize_pack_enqueue(const SymbolTables* st_dev, const PackedTables& t, const TablesOut& o, unsigned char* atom_notes,
                                  unsigned* totals, hipStream_t s) {
    return count_scan_fill(normalize_kernel<false>, normalize_kernel<true>, t.n, RS_THREADS, o, totals, s, t, st_dev, o, atom_notes);
}

}  // namespace mnx
