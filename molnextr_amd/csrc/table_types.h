// table_types.h — the structures of the packed-molecule-table layer as host and device both hold them (internal). No HIP in
// here: the host builders of table_host.h and the plain programs under tools/ see the same text as the kernels. The passes'
// enqueue prototypes are table_passes.h.
#pragma once
#include <stdint.h>

#include "../../include/molnextr_hip.h"

namespace mnx {

// names of the vocabulary's symbol ids as UTF-8 bytes (mnx_set_vocab_text): what graph_pack.hip spells the SMILES with
struct VocabText {
    unsigned char len[256];        // bytes of id i's name, 0..8 (0 beyond the ids that were set)
    unsigned char name[256][8];
};

// the arenas a table writer (mnx_graph_pack, mnx_expand_pack, mnx_smiles_read) fills: the molecule records, then the atom and
// bond records as 64-bit words and the text, each with its capacity in records / bytes. Passed to kernels by value; what is
// done with it is in tables_out.h.
struct TablesOut {
    mnx_mol* mols;
    unsigned long long* atoms;  unsigned atom_cap;
    unsigned long long* bonds;  unsigned bond_cap;
    char* text;                 unsigned text_cap;
};
// the R-group and abbreviation names (mnx_set_symbol_tables), sorted bytewise: what atom_symbol.h looks an atom's symbol up in
struct SymbolTables {
    int n;
    unsigned char len[512];        // bytes of name i, 1..16
    unsigned char kind[512];       // 1 R-group, 2 abbreviation
    unsigned char name[512][16];
};
// the packed tables of mnx_graph_pack as mnx_molfile_pack and mnx_smiles_pack receive them: each table with the number of records
// the caller vouches for (a molecule that points beyond them is refused, atom_symbol.h). Passed to kernels by value.
struct PackedTables {
    const mnx_mol* mols;        int n;
    const mnx_atom* atoms;      unsigned n_atom_records;
    const mnx_bond* bonds;      unsigned n_bond_records;
    const unsigned char* text;  unsigned n_text_bytes;
};
// the fragment library (mnx_set_fragments) as the device holds it: ONE allocation — the table of fragment indices parallel to
// SymbolTables' names, the fragment records, then their atoms, bonds and symbol bytes, each part 8-byte aligned and none empty
// (table_host.h). The host has validated all of it and has sorted every fragment's bonds by (i, j), so the bonds from atom 0 (the
// attachment atom) are the first n_bonds0 of a fragment.
struct FragRec {
    unsigned atom0, bond0, text0;       // where its atoms / bonds / symbol bytes begin in the three arrays
    unsigned short n_atoms, n_bonds, n_bonds0, text_len;    // 1..32 atoms; text_len: its symbols behind one another
};
struct FragView {                       // passed to kernels by value
    const int* frag_of_name;            // [SymbolTables::n] fragment index or -1
    const FragRec* frag;
    const unsigned* atoms;              // sym0 (bytes from the fragment's text0) | sym_len << 16
    const unsigned* bonds;              // i | j << 8 | type << 16
    const unsigned char* text;
};

}  // namespace mnx
