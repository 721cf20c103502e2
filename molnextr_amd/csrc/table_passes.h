// table_passes.h — what the host entry points of engine_tables.hip call: one enqueue function per pass over the packed molecule
// tables, defined in the pass's own .hip (internal). The structures they take are table_types.h.
#pragma once
#include <hip/hip_runtime.h>

#include "table_types.h"

namespace mnx {

struct TokenClasses;    // dec_types.h: the model's token classes, which graph_pack.hip walks the ids with

// graph_pack.hip: the dense outputs of n rows ([n,T] ids, [n,kmax] atoms, [n,kmax,kmax] bonds; the three score pointers all
// null or all set) as packed records (mnx_graph_pack): count, scan and fill, three launches on s
hipError_t graph_pack_enqueue(const TokenClasses* tc_dev, const VocabText* vt_dev, const int* tokens, const int* lens, int n,
                              int T, int kmax, const int* atom_idx, const int* n_atoms, const unsigned char* edges,
                              const double* atom_scores, const double* edge_scores, const double* overall, const TablesOut& o,
                              unsigned* totals, hipStream_t s);
// molfile.hip: the molecules of t as V2000 molfiles behind one another in `out` (mnx_molfile_pack): count, scan and fill, three
// launches on s
hipError_t molfile_pack_enqueue(const SymbolTables* st_dev, const PackedTables& t, const int* scale, int coord_bins,
                                mnx_molfile* files, char* out, unsigned out_cap, unsigned* totals, hipStream_t s);
// smiles.hip: the molecules of t as graph SMILES behind one another in `out`, the atoms' written positions in `order` (may be
// null) (mnx_smiles_pack; marks, MNX_SMILES_MARK_*: with the '@' / '@@' of mnx_smiles_pack_stereo and the '/' '\\' of
// mnx_smiles_pack_marks): count, scan and fill, three launches on s.
// rank set (null otherwise): the same on canonical atom ranks (mnx_smiles_pack_canonical) — one launch in front leaves the ranks
// in `rank` and the symmetry classes in `sym_class` (may be null), then count, scan and fill on those ranks; four launches on s.
// symmetric (rank and sym_class set): the same four launches with the symmetry rule of mnx_smiles_pack_symmetric for the marks,
// every atom's MNX_ATOM_* bits in `atom_marks` (may be null)
hipError_t smiles_pack_enqueue(const SymbolTables* st_dev, const PackedTables& t, unsigned marks, mnx_smiles* recs,
                               unsigned short* order, unsigned short* rank, unsigned short* sym_class, char* out,
                               unsigned out_cap, unsigned* totals, hipStream_t s, bool symmetric = false,
                               unsigned char* atom_marks = nullptr);
// expand.hip: the molecules of t with every abbreviation label that has a fragment replaced by the fragment's atoms and bonds,
// as packed tables of the same record types (mnx_expand_pack): count, scan and fill, three launches on s
hipError_t expand_pack_enqueue(const SymbolTables* st_dev, const FragView& fv, const PackedTables& t, const TablesOut& o,
                               unsigned short* origin, unsigned* totals, hipStream_t s);
// formula.hip: the molecules of t with every condensed-formula label that the search finds a structure for replaced by its atoms and
// bonds, as packed tables of the same record types (mnx_formula_pack): count, scan and fill, three launches on s. max_steps: the
// placements one label's search may try, 0 = MNX_FORMULA_DEFAULT_STEPS.
hipError_t formula_pack_enqueue(const SymbolTables* st_dev, const FragView& fv, const PackedTables& t, const TablesOut& o,
                                unsigned short* origin, unsigned* totals, unsigned max_steps, hipStream_t s);
// main_mol.hip: of every molecule of t the connected component with the most atoms (among equals the one with the lowest atom), the
// other atoms and their bonds dropped, as packed tables of the same record types (mnx_main_pack): count, scan and fill, three
// launches on s
hipError_t main_pack_enqueue(const PackedTables& t, const TablesOut& o, unsigned short* origin, unsigned* totals, hipStream_t s);
// normalize.hip: the molecules of t with one normal spelling per atom — aromatic rings perceived, hydrogens counted, brackets
// dropped where a reader infers them — as packed tables of the same record types (mnx_normalize_pack): count, scan and fill,
// three launches on s; atom_notes (may be null) receives one byte per output atom
hipError_t normalize_pack_enqueue(const SymbolTables* st_dev, const PackedTables& t, const TablesOut& o, unsigned char* atom_notes,
                                  unsigned* totals, hipStream_t s);

// kekulize.hip: the molecules of t with every aromatic system that has a Kekule structure written as one — upper-case atoms,
// double and single bonds — as packed tables of the same record types (mnx_kekulize_pack): count, scan and fill, asynchronous on
// s. max_steps: the pairings one system's search may try, 0 = MNX_KEKULE_DEFAULT_STEPS.
hipError_t kekulize_pack_enqueue(const SymbolTables* st_dev, const PackedTables& t, const TablesOut& o, unsigned char* atom_notes,
                                 unsigned* totals, unsigned max_steps, hipStream_t s);
// fingerprint.hip: of every molecule of t the path fingerprint — 64 words behind one another in `bits`, a record in recs
// (mnx_fingerprint_pack): one launch on s. max_bonds 1 .. 7 and max_steps 1 .. MNX_FP_MAX_STEPS, the defaults resolved
hipError_t fingerprint_pack_enqueue(const SymbolTables* st_dev, const PackedTables& t, mnx_fp* recs, unsigned* bits,
                                    unsigned max_bonds, unsigned max_steps, hipStream_t s);
// the Tanimoto similarity of row r of a and row r of b, n rows of 64 words (mnx_tanimoto; each output may be null): one launch on s
hipError_t tanimoto_enqueue(const unsigned* a, const unsigned* b, int n, unsigned* both, unsigned* either, double* similarity,
                            hipStream_t s);
// nearest.hip: for every row of `queries` the k nearest rows of `library` by that similarity (mnx_tanimoto_search; both, either and
// similarity may be null): scan and merge, two launches on s. The arguments checked, `work` of tanimoto_search_work_bytes at least
size_t tanimoto_search_work_bytes(int nq, unsigned nl, unsigned k);
hipError_t tanimoto_search_enqueue(const unsigned* queries, int nq, const unsigned* library, unsigned nl, unsigned k,
                                   double min_similarity, unsigned flags, unsigned* count, unsigned* index, unsigned* both,
                                   unsigned* either, double* similarity, void* work, hipStream_t s);
// match.hip: for pair p = (pairs[2p], pairs[2p + 1]) whether, how often and where molecule pairs[2p] of q embeds in molecule
// pairs[2p + 1] of t — a record in recs, MNX_MATCH_MAX_QUERY target atoms in maps (mnx_substructure_match): one launch on s.
// max_matches 1 .. 65535 and max_steps 1 .. MNX_MATCH_MAX_STEPS, the defaults resolved
hipError_t match_enqueue(const SymbolTables* st_dev, const PackedTables& q, const PackedTables& t, const unsigned* pairs, int n_pairs,
                         mnx_match* recs, unsigned short* maps, unsigned max_matches, unsigned max_steps, hipStream_t s);
// smiles_read.hip: string b = bytes[offsets[b] .. offsets[b + 1]) read as SMILES into packed tables of mnx_graph_pack's record types
// (mnx_smiles_read): count, scan and fill, three launches on s
hipError_t smiles_read_enqueue(const unsigned char* bytes, unsigned n_bytes, const unsigned* offsets, int n, mnx_read* recs,
                               const TablesOut& o, unsigned* totals, hipStream_t s);
// molfile_read.hip: file b = bytes[offsets[b] .. offsets[b + 1]) read as a V2000 molfile into packed tables of mnx_graph_pack's
// record types (mnx_molfile_read): count, scan and fill, three launches on s. scale: int [n, 2] or null; fit 0 or 1; den =
// cfg.coord_bins - 1
hipError_t molfile_read_enqueue(const unsigned char* bytes, unsigned n_bytes, const unsigned* offsets, int n, const int* scale,
                                int fit, unsigned den, mnx_molread* recs, const TablesOut& o, unsigned* totals, hipStream_t s);

}  // namespace mnx
