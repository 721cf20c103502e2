// main_mol.hip — the main molecule of every packed molecule (mnx_main_pack): what the reference's _keep_main_molecule does to a
// prediction before it is scored — the connected component with the most atoms stays, among equals the one with the lowest atom
// (GetMolFrags lists components by their lowest atom, np.argmax takes the first), salts, counter-ions and stray atoms go — here on
// the packed tables: packed tables in, packed tables of the same record types out, so that every pass and writer runs on the
// result unchanged.
//   count  one workgroup per molecule: the components, their sizes, the main one; the atoms / bonds / text bytes that stay
//          -> mols_out[b]
//   scan   exclusive scan of the three counts over the molecules -> atom0 / bond0 / text0, totals (tables_out.h)
//   fill   one workgroup per molecule: the components again, the kept records behind those offsets
// The rule stands in include/molnextr_hip.h. Selecting and renumbering is the frame of select_pass.h; here is what stays. Every
// atom holds a label in LDS, at first its own index. A round takes every bond record's smaller label to the other end (LDS
// atomicMin) and then lets every atom jump to its label's label; rounds repeat until none changed anything. A label is always an
// atom of the same component and only ever falls, so the fixed point — every atom labelled with its component's lowest atom — is
// the same whatever order the atomics land in: no atomic decides a result. A round moves the lowest label at least one bond
// further, so a molecule of n atoms is done within n rounds; the jumps make it a few in practice. Sizes are integer adds on the
// label's slot, the choice one integer maximum over size << 11 | (2047 - label): both are the same in any order too.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/molnextr_hip.h"
#include "select_pass.h"
#include "table_passes.h"

namespace mnx {
namespace {

template <bool FILL>
__global__ __launch_bounds__(SEL_THREADS) void main_mol_kernel(const PackedTables t, const TablesOut o, unsigned short* __restrict__ origin) {
    __shared__ unsigned label[SEL_MAX];       // an atom's component: its lowest atom
    __shared__ unsigned size[SEL_MAX];        // at a component's lowest atom: its atoms
    __shared__ unsigned short new_index[SEL_MAX];
    __shared__ unsigned scan[2 * SEL_THREADS];
    __shared__ unsigned best;                 // the largest size << 11 | (2047 - label)
    SelectPass<FILL> p(t, o, MNX_MOL_MAIN_REFUSED, origin, new_index);
    if (!p.admitted()) return;
    const int tid = threadIdx.x, na = p.na;
    const size_t nb = p.nb;
    if (!FILL && p.records_refuse()) return;

    for (int a = tid; a < SEL_MAX; a += SEL_THREADS) { label[a] = (unsigned)a; size[a] = 0u; }
    if (tid == 0) best = 0u;
    __syncthreads();

    // ---- components: bond type plays no part, a record with i == j joins nothing ----
    for (int round = 0; round <= na; ++round) {
        int changed = 0;
        for (size_t k = tid; k < nb; k += SEL_THREADS) {
            const BondEnds e = p.bond(k);
            const unsigned li = label[e.i], lj = label[e.j];
            if (li < lj) { atomicMin(&label[e.j], li); changed = 1; }
            else if (lj < li) { atomicMin(&label[e.i], lj); changed = 1; }
        }
        __syncthreads();
        for (int a = tid; a < na; a += SEL_THREADS) {
            const unsigned l = label[a], ll = label[l];
            if (ll < l) { atomicMin(&label[a], ll); changed = 1; }
        }
        if (!__syncthreads_or(changed)) break;
    }

    // ---- sizes, and the choice: the most atoms, among equals the lowest label ----
    for (int a = tid; a < na; a += SEL_THREADS) atomicAdd(&size[label[a]], 1u);
    __syncthreads();
    for (int a = tid; a < na; a += SEL_THREADS)
        if (label[a] == (unsigned)a) atomicMax(&best, size[a] << 11 | (SEL_ATOM_LIMIT - (unsigned)a));
    __syncthreads();
    const unsigned main_label = SEL_ATOM_LIMIT - (best & SEL_ATOM_LIMIT), main_size = best >> 11;

    bool keep[SEL_PER];
#pragma unroll
    for (int q = 0; q < SEL_PER; ++q) {
        const int a = SEL_PER * tid + q;
        keep[q] = a < na && label[a] == main_label;
    }
    p.place_atoms(keep, scan);
    p.place_bonds(scan);
    if (FILL) return;

    int tie = 0;
    for (int a = tid; a < na; a += SEL_THREADS) tie |= label[a] == (unsigned)a && (unsigned)a != main_label && size[a] == main_size;
    tie = __syncthreads_or(tie);
    p.record(p.n_atoms, p.n_bonds, p.n_text, (main_size < (unsigned)na ? MNX_MOL_MAIN_KEPT : 0u) | (tie ? MNX_MOL_MAIN_TIE : 0u));
}

}  // namespace

hipError_t main_pack_enqueue(const PackedTables& t, const TablesOut& o, unsigned short* origin, unsigned* totals, hipStream_t s) {
    return count_scan_fill(main_mol_kernel<false>, main_mol_kernel<true>, t.n, SEL_THREADS, o, totals, s, t, o, origin);
}

}  // namespace mnx
