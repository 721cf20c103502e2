// table_pass.h — one molecule of a pass from packed tables to packed tables in one workgroup, run twice (count, fill;
// tables_out.h): what the frames of respell_pass.h, grow_pass.h and select_pass.h share, once (internal). Who is admitted, what a refusal
// leaves and how count's result is stored is here; who is too large is the frame's.
#pragma once
#include "atom_symbol.h"
#include "tables_out.h"

namespace mnx {

struct BondEnds { unsigned i, j, ty; bool beyond; };     // a bond record's atoms and type; beyond: no bond of the molecule

// Molecule blockIdx.x in one workgroup of a pass, count (FILL = false) or fill. refused: the pass's MNX_MOL_*_REFUSED.
template <bool FILL>
struct TablePass {
    const PackedTables& t;
    const TablesOut& o;
    const unsigned refused;
    const Molecule mol;
    mnx_mol mo;                           // fill: what count and the scan left of the molecule
    const int na;
    const unsigned nb;
    const unsigned long long *A, *B;      // the molecule's atom and bond records as 64-bit words (tables_out.h)

    __device__ __forceinline__ TablePass(const PackedTables& t, const TablesOut& o, unsigned refused)
        : t(t), o(o), refused(refused), mol(admit_molecule(t, blockIdx.x)), na((int)mol.m.n_atoms), nb(mol.m.n_bonds),
          A((const unsigned long long*)mol.A), B((const unsigned long long*)mol.B) {}

    __device__ __forceinline__ const unsigned char* text_in() const { return t.text + mol.m.text0; }
    __device__ __forceinline__ void record(unsigned n_atoms, unsigned n_bonds, unsigned text_len, unsigned flags) const {    // count's result
        if (threadIdx.x == 0)
            store_mol_counts(&o.mols[blockIdx.x], n_atoms, n_bonds, text_len, flags | (mol.m.flags & MNX_MOL_TRUNCATED), mol.m.overall_score);
    }
    // Whether there is anything to do (the same for every thread): count refuses a molecule whose records lie beyond the tables or
    // that is too large for the frame, fill leaves one alone that count refused. A and B are read only behind this.
    __device__ __forceinline__ bool admitted(bool too_large) {
        if (FILL) mo = o.mols[blockIdx.x];
        const bool ok = FILL ? !(mo.flags & refused) : !((mol.flags & PT_BEYOND_TABLES) || too_large);
        if (!FILL && !ok) record(0, 0, 0, refused);
        return ok;
    }
    __device__ __forceinline__ BondEnds bond(size_t k) const {
        const unsigned w = (unsigned)B[2 * k], i = w & 0xffffu, j = w >> 16, ty = (unsigned)(B[2 * k] >> 32) & 0xffu;
        return {i, j, ty, i >= (unsigned)na || j >= (unsigned)na};
    }
    // one barrier: whether a thread found a symbol beyond the text or a bond that is no bond of the molecule; count refuses then
    __device__ __forceinline__ bool refuses(int bad) const {
        bad = __syncthreads_or(bad);
        if (!FILL && bad) record(0, 0, 0, refused);
        return !FILL && bad;
    }
};

}  // namespace mnx
