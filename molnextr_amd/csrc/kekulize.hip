// kekulize.hip — aromatic systems of the packed molecule tables written as Kekule structures (mnx_kekulize_pack): the inverse of
// what normalize.hip perceives, and a pass of respell_pass.h, where its frame is: count, scan and fill, admission and refusal (table_pass.h),
// the slots, the symbols' placing, the records written. The rule stands in include/molnextr_hip.h: a Kekule structure is a
// perfect matching of the atoms that must take a double bond, and the choice among several is this library's own search order,
// not a toolkit's. Inside a workgroup, in count and again in fill: the atoms' interpretation (atom_symbol.h); one stride over the
// bond records for every atom's bond order sum, its type-4 records (the first three as a neighbour list) and the pair of every
// record as a sort key; a bitonic sort of the keys, so that two records of one pair lie side by side; the systems by label
// propagation over the type-4 records between aromatic atoms, with pointer jumping; the needy neighbours of every needy atom;
// then ONE LANE PER SYSTEM runs the search of kekule_search.h, the systems of a molecule side by side, everything in LDS; then
// every atom's new symbol.
#include "respell_pass.h"
#include "table_passes.h"
#include "kekule_search.h"              // behind the HIP runtime, which the tools' host build of it does without

namespace mnx {
namespace {

static_assert(kekule::NONE >= 999u && kekule::NONE < (unsigned)RS_MAX, "an atom index that no atom has, in 10 bits");

// ---- an atom's state word ----
//   bits 0-3 H count, bit 4 aromatic atom, bit 5 needy, bit 6 one of the atom's records blocks its system,
//   on a system's lowest atom: bit 7 the system is blocked, bits 8-9 what the search returned (kekule::OK / NO_MATCHING / LIMIT)
constexpr unsigned ST_AROMATIC = 1u << 4, ST_NEEDY = 1u << 5, ST_BLOCKS = 1u << 6, ST_BLOCKED = 1u << 7, ST_RESULT = 8;
__device__ __forceinline__ unsigned st_result(unsigned s) { return s >> ST_RESULT & 3u; }

// v of the needy rule for (element, charge); 0 for a pair the rule does not list
__device__ __forceinline__ unsigned needy_valence(unsigned el, int q) {
    if (el == EL('C')) return q == 0 ? 4u : (q == 1 || q == -1) ? 3u : 0u;
    if (el == EL('N') || el == EL('P')) return q == 0 ? 3u : q == 1 ? 4u : 0u;
    if (el == EL('B')) return q == 0 ? 3u : q == -1 ? 4u : 0u;
    if (el == EL('A', 's')) return q == 0 ? 3u : 0u;
    if (el == EL('O') || el == EL('S') || el == EL('S', 'e')) return q == 0 ? 2u : q == 1 ? 3u : 0u;
    return 0u;
}

template <bool FILL>
__global__ __launch_bounds__(RS_THREADS) void kekulize_kernel(
        const PackedTables t, const SymbolTables* __restrict__ stab, const TablesOut o, unsigned char* __restrict__ notes,
        const unsigned max_steps) {
    __shared__ unsigned info[RS_MAX], elem[RS_MAX];
    __shared__ unsigned cnt[RS_MAX];      // type-4 records at the atom: hands out the slots of nbr3
    __shared__ unsigned acc[RS_MAX];      // bond order sum
    __shared__ unsigned st[RS_MAX];
    __shared__ unsigned nbr3[3 * RS_MAX]; // the first three type-4 neighbours; later the needy neighbours of a needy atom
    __shared__ unsigned keys[RS_MAX];     // per bond record: lower atom << 10 | higher atom, sorted
    __shared__ unsigned edge[RS_MAX];     // per bond record: i | j << 10 of a type-4 record between two aromatic atoms, else RS_NONE
    __shared__ unsigned label[RS_MAX];    // an aromatic atom's system: the lowest atom of its component
    __shared__ unsigned searched[RS_MAX]; // the system a needy atom is searched in, kekule::NONE for every other atom
    __shared__ unsigned state[RS_MAX];    // the search's word per needy atom (kekule_search.h)
    __shared__ unsigned scan[2 * RS_THREADS];
    const int tid = threadIdx.x;
    RespellPass<FILL> p(t, o, MNX_MOL_KEKULIZE_REFUSED);
    if (!p.admitted()) return;
    const int na = p.na, nb = p.nb;

    // ---- the atoms as the writers read them; per atom its bond order sum and its first three type-4 records ----
    int bad = interpret_atoms<RS_MAX, RS_THREADS>(t, stab, p.mol, info, elem);
    for (int a = tid; a < RS_MAX; a += RS_THREADS) {
        cnt[a] = 0; acc[a] = 0; st[a] = 0;
        nbr3[3 * a] = nbr3[3 * a + 1] = nbr3[3 * a + 2] = RS_NONE;
        keys[a] = RS_NONE; edge[a] = RS_NONE; label[a] = RS_NONE; searched[a] = kekule::NONE;
    }
    __syncthreads();
    auto aromatic_atom = [&](unsigned a) { return info_cls(info[a]) == CLS_ATOM && info_aromatic(info[a]); };
    int any = 0;
    for (int a = tid; a < na; a += RS_THREADS) any |= aromatic_atom((unsigned)a);
    for (int k = tid; k < nb; k += RS_THREADS) {
        const auto [i, j, ty, beyond] = p.bond(k);
        if (beyond) { bad = 1; continue; }
        const unsigned order = (ty == 1 || ty == 4 || ty == 5 || ty == 6) ? 1u : (ty == 2 || ty == 3) ? ty : 0u;
        unsigned fi = (order == 0 || i == j) ? ST_BLOCKS : 0u, fj = fi;     // no class of a bond, or from an atom to itself
        if (ty == 4 && i != j) {
            const bool ai = aromatic_atom(i), aj = aromatic_atom(j);
            if (!aj) fi |= ST_BLOCKS;     // the other end is no aromatic atom
            if (!ai) fj |= ST_BLOCKS;
            if (ai && aj) edge[k] = i | j << 10;
            hand_out_slots(cnt, nbr3, i, j, j, i);
        }
        if (fi) atomicOr(&st[i], fi);
        if (fj) atomicOr(&st[j], fj);
        atomicAdd(&acc[i], order);        // a sum does not depend on the order of its terms; a record from an atom to itself
        atomicAdd(&acc[j], order);        // counts at both of its ends
        keys[k] = min(i, j) << 10 | max(i, j);
    }
    if (p.refuses(bad)) return;           // a symbol beyond the text or a bond that is no bond of the molecule
    any = __syncthreads_or(any);

    if (any) {                            // the same for every thread; without an aromatic atom everything is copied
        // ---- two records of one pair of atoms: side by side behind a bitonic sort of the keys ----
        int width = 2;
        while (width < nb) width <<= 1;
        for (int run = 2; run <= width; run <<= 1)
            for (int d = run >> 1; d > 0; d >>= 1) {
                for (int x = tid; x < width; x += RS_THREADS) {
                    const int y = x ^ d;
                    if (y > x) {
                        const unsigned p = keys[x], q = keys[y];
                        if ((p > q) == ((x & run) == 0)) { keys[x] = q; keys[y] = p; }
                    }
                }
                __syncthreads();
            }
        for (int x = tid; x + 1 < width; x += RS_THREADS) {
            const unsigned p = keys[x];
            if (p != RS_NONE && p == keys[x + 1]) {
                atomicOr(&st[p >> 10], ST_BLOCKS);
                atomicOr(&st[p & 1023u], ST_BLOCKS);
            }
        }
        __syncthreads();

        // ---- every aromatic atom: hydrogens, whether it is needy, its three slots in ascending order, a system of its own ----
        for (int a = tid; a < na; a += RS_THREADS) {
            if (!aromatic_atom((unsigned)a)) { st[a] = 0; continue; }
            const unsigned w = info[a], el = elem[a] & 0xffffu, bo = acc[a];
            unsigned e0, e1, e2;
            sort_slots(&nbr3[3 * a], e0, e1, e2);
            const unsigned h = (w & 4u) ? (unsigned)info_h(w) : el == EL('C') ? (bo < 3 ? 3 - bo : 0u) : 0u;
            const unsigned v = needy_valence(el, info_charge(w));
            const bool needy = v != 0 && v == bo + h + 1;
            st[a] = h | ST_AROMATIC | (needy ? ST_NEEDY : 0u) | ((st[a] & ST_BLOCKS) || cnt[a] > 3 ? ST_BLOCKS : 0u);
            label[a] = (unsigned)a;
        }
        __syncthreads();

        // ---- systems: every atom's label falls to the lowest atom of its component; a label is always an atom of the component,
        //      so the minimum the atomics take is the same whatever their order. At most one round per atom, a few in practice ----
        for (int round = 0; round < RS_MAX; ++round) {
            int changed = 0;
            for (int k = tid; k < nb; k += RS_THREADS) {
                const unsigned e = edge[k];
                if (e == RS_NONE) continue;
                const unsigned i = e & 1023u, j = e >> 10, li = label[i], lj = label[j];
                if (li < lj) { atomicMin(&label[j], li); changed = 1; }
                else if (lj < li) { atomicMin(&label[i], lj); changed = 1; }
            }
            __syncthreads();
            for (int a = tid; a < na; a += RS_THREADS) {
                const unsigned l = label[a];
                if (l == RS_NONE) continue;
                const unsigned ll = label[l];
                if (ll < l) { atomicMin(&label[a], ll); changed = 1; }
            }
            if (!__syncthreads_or(changed)) break;
        }
        for (int a = tid; a < na; a += RS_THREADS)
            if ((st[a] & (ST_AROMATIC | ST_BLOCKS)) == (ST_AROMATIC | ST_BLOCKS)) atomicOr(&st[label[a]], ST_BLOCKED);
        __syncthreads();

        // ---- a needy atom of a system that is not blocked: the system it is searched in and its needy neighbours, ascending. All
        //      its type-4 records are in its three slots, go to aromatic atoms of its system and to different ones ----
        for (int a = tid; a < na; a += RS_THREADS) {
            const unsigned s = st[a];
            const bool in = (s & ST_NEEDY) && !(st[label[a]] & ST_BLOCKED);
            unsigned e[3] = {kekule::NONE, kekule::NONE, kekule::NONE}, n = 0;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const unsigned x = nbr3[3 * a + q];
                const bool keep = in && x != RS_NONE && (st[x] & ST_NEEDY);
                if (keep && n == 0) e[0] = x;
                if (keep && n == 1) e[1] = x;
                if (keep && n == 2) e[2] = x;
                n += keep;
            }
            nbr3[3 * a] = e[0]; nbr3[3 * a + 1] = e[1]; nbr3[3 * a + 2] = e[2];
            if (in) searched[a] = label[a];
        }
        __syncthreads();

        // ---- the search: one lane per system that is not blocked, serial inside a system ----
        for (int a = tid; a < na; a += RS_THREADS) {
            const unsigned s = st[a];
            if (!(s & ST_AROMATIC) || label[a] != (unsigned)a || (s & ST_BLOCKED)) continue;
            unsigned steps;
            st[a] = s | kekule::search((unsigned)a, (unsigned)na, searched, nbr3, state, max_steps, &steps) << ST_RESULT;
        }
        __syncthreads();
    }

    // whether the aromatic atom a was rewritten: its system is not blocked and has a matching
    auto rewritten = [&](unsigned a) {
        const unsigned sr = st[label[a]];
        return !(sr & ST_BLOCKED) && st_result(sr) == kekule::OK;
    };

    // ---- every atom's new symbol; an atom that is not aromatic and one of a system left as it came keep theirs ----
    p.atoms(scan, notes, MNX_NOTE_KEKULIZED, MNX_MOL_KEKULIZED, MNX_NOTE_KEKULE_LEFT, MNX_MOL_KEKULE_LEFT,
            [&](int a, Spelled& sym, unsigned& note) {
                const unsigned s = st[a], w = info[a];
                if (!(s & ST_AROMATIC) || !rewritten((unsigned)a)) {
                    if (!(s & ST_AROMATIC)) note = MNX_NOTE_COPIED;
                    else {
                        const unsigned sr = st[label[a]];
                        note = st_h(s) | MNX_NOTE_KEKULE_LEFT | (!(sr & ST_BLOCKED) && st_result(sr) == kekule::LIMIT ? MNX_NOTE_KEKULE_LIMIT : 0u);
                    }
                    return true;
                }
                const unsigned el = elem[a] & 0xffffu, bo = acc[a] + ((s & ST_NEEDY) ? 1u : 0u);     // a needy atom took one double bond
                spell_packed(sym, el, false, info_num(w), st_h(s), info_charge(w), implicit_h(el, bo));
                note = st_h(s) | MNX_NOTE_KEKULIZED;
                return false;
            });
    if (!FILL) return;
    // ---- the bonds: a type-4 record of a rewritten system is double between partners and single otherwise ----
    p.bonds([&](int k, unsigned) {
        const unsigned e = edge[k];
        if (e == RS_NONE || !rewritten(e & 1023u)) return 0ull;
        const unsigned i = e & 1023u, j = e >> 10;
        return (st[i] & ST_NEEDY) && kekule::partner(state[i]) == j ? 2ull : 1ull;
    });
}

}  // namespace

hipError_t kekulize_pack_enqueue(const SymbolTables* st_dev, const PackedTables& t, const TablesOut& o, unsigned char* atom_notes,
                                 unsigned* totals, unsigned max_steps, hipStream_t s) {
    const unsigned steps = max_steps ? max_steps : MNX_KEKULE_DEFAULT_STEPS;
    return count_scan_fill(kekulize_kernel<false>, kekulize_kernel<true>, t.n, RS_THREADS, o, totals, s, t, st_dev, o, atom_notes, steps);
}

}  // namespace mnx
