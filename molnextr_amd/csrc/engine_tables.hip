// engine_tables.hip — host side of libmolnextr_hip.so, the packed-molecule-table layer of include/molnextr_hip.h: the three
// setters of its name and fragment tables (their host work is table_host.h) and one entry point per pass (table_passes.h). Of the
// engine they read the device, the error string, cfg.coord_bins / sym_offset and the tables the setters uploaded.
#include <cstring>
#include <memory>

#include "engine_impl.h"
#include "table_host.h"
#include "table_passes.h"

using namespace mnx;

extern "C" {

int mnx_set_vocab_text(mnx_engine* h, const char* bytes, const uint32_t* offsets, int32_t n) {
    if (!h) return MNX_ERR_INVALID_ARG;
    VocabText vt;
    if (const std::string why = build_vocab_text(bytes, offsets, n, h->cfg.sym_offset, &vt); !why.empty()) { h->err = why; return MNX_ERR_INVALID_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy(h->vt_dev, &vt, sizeof(vt), hipMemcpyHostToDevice));
    h->have_vt = true;
    return MNX_OK;
}

// The caller's four input tables as every pass receives them
static PackedTables packed_tables(const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records, const mnx_bond* bonds,
                                  uint32_t n_bond_records, const char* text, uint32_t n_text_bytes) {
    return PackedTables{mols, n, atoms, n_atom_records, bonds, n_bond_records, (const unsigned char*)text, n_text_bytes};
}

// The output tables of mnx_graph_pack, mnx_expand_pack and mnx_smiles_read with their `totals`: what each tests of them
static TablesOut tables_out(mnx_mol* mols, mnx_atom* atoms, uint32_t atom_cap, mnx_bond* bonds, uint32_t bond_cap, char* text,
                            uint32_t text_cap) {
    return TablesOut{mols, (unsigned long long*)atoms, atom_cap, (unsigned long long*)bonds, bond_cap, text, text_cap};
}
static bool tables_out_null(const TablesOut& o, const uint32_t* totals) {
    return !o.mols || !totals || (!o.atoms && o.atom_cap) || (!o.bonds && o.bond_cap) || (!o.text && o.text_cap);
}
static bool tables_out_skew(const TablesOut& o, const uint32_t* totals) {
    return ((((uintptr_t)o.mols | (uintptr_t)o.atoms | (uintptr_t)o.bonds) & 7) | ((uintptr_t)totals & 3)) != 0;
}

int mnx_graph_pack(mnx_engine* h, const int32_t* tokens, const int32_t* lengths, int32_t n, int32_t T,
                   const int32_t* atom_idx, const int32_t* n_atoms, const uint8_t* edges, int32_t kmax,
                   const double* atom_scores, const double* edge_scores, const double* overall_score, mnx_mol* mols,
                   mnx_atom* atoms, uint32_t atom_cap, mnx_bond* bonds, uint32_t bond_cap, char* text, uint32_t text_cap,
                   uint32_t* totals, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    const TablesOut o = tables_out(mols, atoms, atom_cap, bonds, bond_cap, text, text_cap);
    if (!tokens || !lengths || !atom_idx || !n_atoms || !edges || tables_out_null(o, totals)) {
        h->err = "mnx_graph_pack: null pointer";
        return MNX_ERR_INVALID_ARG;
    }
    if (n < 1 || n > 65536 || T < 1 || T > 512 || kmax < 1 || kmax > h->db.kmax) {
        h->err = "mnx_graph_pack: 1 <= n <= 65536, 1 <= T <= 512 and 1 <= kmax <= cfg.max_atoms required";
        return MNX_ERR_INVALID_ARG;
    }
    const int n_scores = (atom_scores != nullptr) + (edge_scores != nullptr) + (overall_score != nullptr);
    if (n_scores != 0 && n_scores != 3) {
        h->err = "mnx_graph_pack: atom_scores, edge_scores and overall_score go together (all three or none)";
        return MNX_ERR_INVALID_ARG;
    }
    if (tables_out_skew(o, totals)) {
        h->err = "mnx_graph_pack: mols, atoms and bonds must be 8-byte aligned, totals 4-byte";
        return MNX_ERR_INVALID_ARG;
    }
    if (!h->have_tc) { h->err = "mnx_graph_pack: call mnx_set_token_classes first"; return MNX_ERR_INVALID_ARG; }
    if (!h->have_vt) { h->err = "mnx_graph_pack: call mnx_set_vocab_text first"; return MNX_ERR_INVALID_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, graph_pack_enqueue(h->tc_dev, h->vt_dev, tokens, lengths, n, T, kmax, atom_idx, n_atoms, edges, atom_scores,
                                 edge_scores, overall_score, o, totals, (hipStream_t)stream));
    return MNX_OK;
}

int mnx_set_symbol_tables(mnx_engine* h, const char* bytes, const uint32_t* offsets, const uint8_t* kinds, int32_t n) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto st = std::make_unique<SymbolTables>();
    if (const std::string why = build_symbol_tables(bytes, offsets, kinds, n, st.get()); !why.empty()) { h->err = why; return MNX_ERR_INVALID_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy(h->st_dev, st.get(), sizeof(SymbolTables), hipMemcpyHostToDevice));
    h->have_st = true;
    h->st_n = n;
    memcpy(h->st_kind, st->kind, sizeof(h->st_kind));
    h->have_frag = false;       // a fragment table is parallel to the names it was set for
    return MNX_OK;
}

int mnx_set_fragments(mnx_engine* h, const mnx_mol* frags, int32_t n_frags, const mnx_atom* atoms, uint32_t na, const mnx_bond* bonds,
                      uint32_t nb, const char* text, uint32_t nt, const int32_t* frag_of_name, int32_t n_names) {
    if (!h) return MNX_ERR_INVALID_ARG;
    if (!h->have_st) { h->err = "mnx_set_fragments: call mnx_set_symbol_tables first"; return MNX_ERR_INVALID_ARG; }
    FragImage img;
    if (const std::string why = build_fragments(frags, n_frags, atoms, na, bonds, nb, text, nt, frag_of_name, n_names, h->st_kind, h->st_n, &img);
        !why.empty()) {
        h->err = why;
        return MNX_ERR_INVALID_ARG;
    }
    const size_t total = img.blob.size();
    void* dev = nullptr;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMalloc(&dev, total));
    if (hipError_t e = hipMemcpy(dev, img.blob.data(), total, hipMemcpyHostToDevice); e != hipSuccess) {
        hipFree(dev);
        h->err = std::string("mnx_set_fragments: hipMemcpy: ") + hipGetErrorString(e);
        return MNX_ERR_HIP;
    }
    if (h->frag_dev) {          // an earlier table may still be read by launches in flight
        (void)hipDeviceSynchronize();
        hipFree(h->frag_dev);
    }
    h->frag_dev = dev;
    const unsigned char* d = (const unsigned char*)dev;
    h->fv = FragView{(const int*)(d + img.off[0]), (const FragRec*)(d + img.off[1]), (const unsigned*)(d + img.off[2]),
                     (const unsigned*)(d + img.off[3]), d + img.off[4]};
    h->have_frag = true;
    return MNX_OK;
}

// What mnx_molfile_pack, mnx_expand_pack, mnx_normalize_pack, mnx_kekulize_pack and the five mnx_smiles_pack* test before they launch, in
// the order in which a call refused for two reasons reports them. Its own pointers (outs_null, outs_skew) the entry point tests; `aligned` ends its alignment message.
static int check_packed_tables(mnx_engine* h, const char* fn, const PackedTables& t, bool outs_null, bool outs_skew,
                               const char* aligned, bool reads_symbols = true) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const std::string& m) { h->err = std::string(fn) + ": " + m; return MNX_ERR_INVALID_ARG; };
    if (!t.mols || (!t.atoms && t.n_atom_records) || (!t.bonds && t.n_bond_records) || (!t.text && t.n_text_bytes) || outs_null)
        return bad("null pointer");
    if (t.n < 1 || t.n > 65536) return bad("1 <= n <= 65536 required");
    if ((((uintptr_t)t.mols | (uintptr_t)t.atoms | (uintptr_t)t.bonds) & 7) || outs_skew)
        return bad(std::string("mols, atoms and bonds must be 8-byte aligned, ") + aligned);
    if (reads_symbols && !h->have_st) return bad("call mnx_set_symbol_tables first");
    return MNX_OK;
}

int mnx_molfile_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                     const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes,
                     const int32_t* scale, mnx_molfile* files, char* out, uint32_t out_cap, uint32_t* totals, void* stream) {
    const PackedTables t = packed_tables(mols, n, atoms, n_atom_records, bonds, n_bond_records, text, n_text_bytes);
    if (int rc = check_packed_tables(h, "mnx_molfile_pack", t, !files || !totals || (!out && out_cap),
                                     (((uintptr_t)files | (uintptr_t)totals | (uintptr_t)scale) & 3) != 0, "files, scale and totals 4-byte"))
        return rc;
    if (h->cfg.coord_bins < 2) { h->err = "mnx_molfile_pack: cfg.coord_bins must be at least 2"; return MNX_ERR_INVALID_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, molfile_pack_enqueue(h->st_dev, t, scale, h->cfg.coord_bins, files, out, out_cap, totals, (hipStream_t)stream));
    return MNX_OK;
}

// mnx_expand_pack and mnx_formula_pack (formula, with its max_steps): one check, one way to the pass's three launches
static int grow_pack(mnx_engine* h, const char* fn, const PackedTables& t, const TablesOut& o, uint16_t* origin, uint32_t* totals,
                     void* stream, bool formula = false, uint32_t max_steps = 0) {
    if (int rc = check_packed_tables(h, fn, t, tables_out_null(o, totals), tables_out_skew(o, totals) || ((uintptr_t)origin & 1) != 0,
                                     "the output tables too, totals 4-byte, origin 2-byte"))
        return rc;
    if (!h->have_frag) { h->err = std::string(fn) + ": call mnx_set_fragments first"; return MNX_ERR_INVALID_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    if (formula) HIPCHK(h, formula_pack_enqueue(h->st_dev, h->fv, t, o, origin, totals, max_steps, (hipStream_t)stream));
    else HIPCHK(h, expand_pack_enqueue(h->st_dev, h->fv, t, o, origin, totals, (hipStream_t)stream));
    return MNX_OK;
}

int mnx_expand_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                    const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_mol* mols_out,
                    mnx_atom* atoms_out, uint32_t atom_cap, mnx_bond* bonds_out, uint32_t bond_cap, char* text_out, uint32_t text_cap,
                    uint16_t* origin, uint32_t* totals, void* stream) {
    const PackedTables t = packed_tables(mols, n, atoms, n_atom_records, bonds, n_bond_records, text, n_text_bytes);
    const TablesOut o = tables_out(mols_out, atoms_out, atom_cap, bonds_out, bond_cap, text_out, text_cap);
    return grow_pack(h, "mnx_expand_pack", t, o, origin, totals, stream);
}

int mnx_formula_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                     const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_mol* mols_out,
                     mnx_atom* atoms_out, uint32_t atom_cap, mnx_bond* bonds_out, uint32_t bond_cap, char* text_out, uint32_t text_cap,
                     uint16_t* origin, uint32_t* totals, uint32_t max_steps, void* stream) {
    const PackedTables t = packed_tables(mols, n, atoms, n_atom_records, bonds, n_bond_records, text, n_text_bytes);
    const TablesOut o = tables_out(mols_out, atoms_out, atom_cap, bonds_out, bond_cap, text_out, text_cap);
    return grow_pack(h, "mnx_formula_pack", t, o, origin, totals, stream, true, max_steps);
}

// mnx_main_pack reads no symbol: it needs neither symbol tables nor fragments
int mnx_main_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                  const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_mol* mols_out,
                  mnx_atom* atoms_out, uint32_t atom_cap, mnx_bond* bonds_out, uint32_t bond_cap, char* text_out, uint32_t text_cap,
                  uint16_t* origin, uint32_t* totals, void* stream) {
    const PackedTables t = packed_tables(mols, n, atoms, n_atom_records, bonds, n_bond_records, text, n_text_bytes);
    const TablesOut o = tables_out(mols_out, atoms_out, atom_cap, bonds_out, bond_cap, text_out, text_cap);
    if (int rc = check_packed_tables(h, "mnx_main_pack", t, tables_out_null(o, totals), tables_out_skew(o, totals) || ((uintptr_t)origin & 1) != 0,
                                     "the output tables too, totals 4-byte, origin 2-byte", false))
        return rc;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, main_pack_enqueue(t, o, origin, totals, (hipStream_t)stream));
    return MNX_OK;
}

// mnx_normalize_pack and mnx_kekulize_pack (kekulize, with its max_steps): one check, one way to the pass's three launches
static int respell_pack(mnx_engine* h, const char* fn, const PackedTables& t, const TablesOut& o, uint8_t* atom_notes, uint32_t* totals,
                        void* stream, bool kekulize = false, uint32_t max_steps = 0) {
    if (int rc = check_packed_tables(h, fn, t, tables_out_null(o, totals), tables_out_skew(o, totals), "the output tables too, totals 4-byte"))
        return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if (kekulize) HIPCHK(h, kekulize_pack_enqueue(h->st_dev, t, o, atom_notes, totals, max_steps, (hipStream_t)stream));
    else HIPCHK(h, normalize_pack_enqueue(h->st_dev, t, o, atom_notes, totals, (hipStream_t)stream));
    return MNX_OK;
}

int mnx_normalize_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                       const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_mol* mols_out,
                       mnx_atom* atoms_out, uint32_t atom_cap, mnx_bond* bonds_out, uint32_t bond_cap, char* text_out,
                       uint32_t text_cap, uint8_t* atom_notes, uint32_t* totals, void* stream) {
    const PackedTables t = packed_tables(mols, n, atoms, n_atom_records, bonds, n_bond_records, text, n_text_bytes);
    const TablesOut o = tables_out(mols_out, atoms_out, atom_cap, bonds_out, bond_cap, text_out, text_cap);
    return respell_pack(h, "mnx_normalize_pack", t, o, atom_notes, totals, stream);
}

int mnx_kekulize_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                      const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_mol* mols_out,
                      mnx_atom* atoms_out, uint32_t atom_cap, mnx_bond* bonds_out, uint32_t bond_cap, char* text_out,
                      uint32_t text_cap, uint8_t* atom_notes, uint32_t* totals, uint32_t max_steps, void* stream) {
    const PackedTables t = packed_tables(mols, n, atoms, n_atom_records, bonds, n_bond_records, text, n_text_bytes);
    const TablesOut o = tables_out(mols_out, atoms_out, atom_cap, bonds_out, bond_cap, text_out, text_cap);
    return respell_pack(h, "mnx_kekulize_pack", t, o, atom_notes, totals, stream, true, max_steps);
}

int mnx_smiles_read(mnx_engine* h, const char* bytes, uint32_t n_bytes, const uint32_t* offsets, int32_t n, mnx_mol* mols,
                    mnx_read* recs, mnx_atom* atoms, uint32_t atom_cap, mnx_bond* bonds, uint32_t bond_cap, char* text,
                    uint32_t text_cap, uint32_t* totals, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const char* m) { h->err = std::string("mnx_smiles_read: ") + m; return MNX_ERR_INVALID_ARG; };
    const TablesOut o = tables_out(mols, atoms, atom_cap, bonds, bond_cap, text, text_cap);
    if ((!bytes && n_bytes) || !offsets || !recs || tables_out_null(o, totals)) return bad("null pointer");
    if (n < 1 || n > 65536) return bad("1 <= n <= 65536 required");
    if (tables_out_skew(o, totals) || (((uintptr_t)recs | (uintptr_t)offsets) & 3))
        return bad("mols, atoms and bonds must be 8-byte aligned, recs, offsets and totals 4-byte");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, smiles_read_enqueue((const unsigned char*)bytes, n_bytes, offsets, n, recs, o, totals, (hipStream_t)stream));
    return MNX_OK;
}

int mnx_molfile_read(mnx_engine* h, const char* bytes, uint32_t n_bytes, const uint32_t* offsets, int32_t n,
                     const int32_t* scale, int32_t fit, mnx_mol* mols, mnx_molread* recs, mnx_atom* atoms, uint32_t atom_cap,
                     mnx_bond* bonds, uint32_t bond_cap, char* text, uint32_t text_cap, uint32_t* totals, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const char* m) { h->err = std::string("mnx_molfile_read: ") + m; return MNX_ERR_INVALID_ARG; };
    const TablesOut o = tables_out(mols, atoms, atom_cap, bonds, bond_cap, text, text_cap);
    if ((!bytes && n_bytes) || !offsets || !recs || tables_out_null(o, totals)) return bad("null pointer");
    if (n < 1 || n > 65536) return bad("1 <= n <= 65536 required");
    if (fit != 0 && fit != 1) return bad("fit must be 0 or 1");
    if (fit && scale) return bad("fit = 1 takes no scale");
    if (tables_out_skew(o, totals) || (((uintptr_t)recs | (uintptr_t)offsets | (uintptr_t)scale) & 3))
        return bad("mols, atoms and bonds must be 8-byte aligned, recs, offsets, scale and totals 4-byte");
    if (h->cfg.coord_bins < 2) return bad("cfg.coord_bins must be at least 2");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, molfile_read_enqueue((const unsigned char*)bytes, n_bytes, offsets, n, scale, fit, (unsigned)h->cfg.coord_bins - 1u, recs, o,
                                   totals, (hipStream_t)stream));
    return MNX_OK;
}

// mnx_smiles_pack, mnx_smiles_pack_stereo, mnx_smiles_pack_marks, mnx_smiles_pack_canonical and mnx_smiles_pack_symmetric: one
// check, one enqueue path, a pair of kernels per set of marks; canonical: on the ranks that one more kernel in front of them
// leaves in `rank`; symmetric: canonical with the symmetry rule, which needs `sym_class` too
static int smiles_pack(mnx_engine* h, const char* fn, uint32_t marks, const PackedTables& t, mnx_smiles* recs, uint16_t* order,
                       char* out, uint32_t out_cap, uint32_t* totals, void* stream, bool canonical = false, uint16_t* rank = nullptr,
                       uint16_t* sym_class = nullptr, bool symmetric = false, uint8_t* atom_marks = nullptr) {
    if (int rc = check_packed_tables(h, fn, t, !recs || !totals || (!out && out_cap) || (canonical && !rank) || (symmetric && !sym_class),
                                     (((uintptr_t)recs | (uintptr_t)totals) & 3) != 0 ||
                                         (((uintptr_t)order | (uintptr_t)rank | (uintptr_t)sym_class) & 1) != 0,
                                     canonical ? "recs and totals 4-byte, order, rank and sym_class 2-byte" : "recs and totals 4-byte, order 2-byte"))
        return rc;
    if (marks & ~(MNX_SMILES_MARK_TETRAHEDRAL | MNX_SMILES_MARK_DOUBLE_BOND)) {
        h->err = std::string(fn) + ": marks may hold MNX_SMILES_MARK_TETRAHEDRAL and MNX_SMILES_MARK_DOUBLE_BOND only";
        return MNX_ERR_INVALID_ARG;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, smiles_pack_enqueue(h->st_dev, t, marks, recs, order, rank, sym_class, out, out_cap, totals, (hipStream_t)stream, symmetric,
                                  atom_marks));
    return MNX_OK;
}

int mnx_smiles_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                    const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_smiles* recs,
                    uint16_t* order, char* out, uint32_t out_cap, uint32_t* totals, void* stream) {
    const PackedTables t = packed_tables(mols, n, atoms, n_atom_records, bonds, n_bond_records, text, n_text_bytes);
    return smiles_pack(h, "mnx_smiles_pack", 0u, t, recs, order, out, out_cap, totals, stream);
}

int mnx_smiles_pack_stereo(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                           const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes,
                           mnx_smiles* recs, uint16_t* order, char* out, uint32_t out_cap, uint32_t* totals, void* stream) {
    const PackedTables t = packed_tables(mols, n, atoms, n_atom_records, bonds, n_bond_records, text, n_text_bytes);
    return smiles_pack(h, "mnx_smiles_pack_stereo", MNX_SMILES_MARK_TETRAHEDRAL, t, recs, order, out, out_cap, totals, stream);
}

int mnx_smiles_pack_marks(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                          const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes,
                          mnx_smiles* recs, uint16_t* order, char* out, uint32_t out_cap, uint32_t* totals, uint32_t marks,
                          void* stream) {
    const PackedTables t = packed_tables(mols, n, atoms, n_atom_records, bonds, n_bond_records, text, n_text_bytes);
    return smiles_pack(h, "mnx_smiles_pack_marks", marks, t, recs, order, out, out_cap, totals, stream);
}

int mnx_smiles_pack_canonical(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                              const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes,
                              mnx_smiles* recs, uint16_t* order, uint16_t* rank, uint16_t* sym_class, char* out,
                              uint32_t out_cap, uint32_t* totals, uint32_t marks, void* stream) {
    const PackedTables t = packed_tables(mols, n, atoms, n_atom_records, bonds, n_bond_records, text, n_text_bytes);
    return smiles_pack(h, "mnx_smiles_pack_canonical", marks, t, recs, order, out, out_cap, totals, stream, true, rank, sym_class);
}

int mnx_smiles_pack_symmetric(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                              const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes,
                              mnx_smiles* recs, uint16_t* order, uint16_t* rank, uint16_t* sym_class, uint8_t* atom_marks,
                              char* out, uint32_t out_cap, uint32_t* totals, uint32_t marks, void* stream) {
    const PackedTables t = packed_tables(mols, n, atoms, n_atom_records, bonds, n_bond_records, text, n_text_bytes);
    return smiles_pack(h, "mnx_smiles_pack_symmetric", marks, t, recs, order, out, out_cap, totals, stream, true, rank, sym_class,
                       true, atom_marks);
}

int mnx_fingerprint_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                         const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_fp* recs,
                         uint32_t* bits, uint32_t max_bonds, uint32_t max_steps, void* stream) {
    const PackedTables t = packed_tables(mols, n, atoms, n_atom_records, bonds, n_bond_records, text, n_text_bytes);
    if (int rc = check_packed_tables(h, "mnx_fingerprint_pack", t, !recs || !bits, (((uintptr_t)recs | (uintptr_t)bits) & 3) != 0,
                                     "recs and bits 4-byte"))
        return rc;
    if (max_bonds > MNX_FP_MAX_BONDS) { h->err = "mnx_fingerprint_pack: max_bonds must be 1 to 7, or 0 for 7"; return MNX_ERR_INVALID_ARG; }
    if (max_steps > MNX_FP_MAX_STEPS) {
        h->err = "mnx_fingerprint_pack: max_steps must not exceed MNX_FP_MAX_STEPS (1048576)";
        return MNX_ERR_INVALID_ARG;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, fingerprint_pack_enqueue(h->st_dev, t, recs, bits, max_bonds ? max_bonds : MNX_FP_MAX_BONDS,
                                       max_steps ? max_steps : MNX_FP_DEFAULT_STEPS, (hipStream_t)stream));
    return MNX_OK;
}

int mnx_substructure_match(mnx_engine* h,
                           const mnx_mol* q_mols, int32_t nq, const mnx_atom* q_atoms, uint32_t q_atom_records, const mnx_bond* q_bonds,
                           uint32_t q_bond_records, const char* q_text, uint32_t q_text_bytes,
                           const mnx_mol* t_mols, int32_t nt, const mnx_atom* t_atoms, uint32_t t_atom_records, const mnx_bond* t_bonds,
                           uint32_t t_bond_records, const char* t_text, uint32_t t_text_bytes,
                           const uint32_t* pairs, int32_t n_pairs, mnx_match* recs, uint16_t* maps,
                           uint32_t max_matches, uint32_t max_steps, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const char* m) { h->err = std::string("mnx_substructure_match: ") + m; return MNX_ERR_INVALID_ARG; };
    const PackedTables q = packed_tables(q_mols, nq, q_atoms, q_atom_records, q_bonds, q_bond_records, q_text, q_text_bytes);
    const PackedTables t = packed_tables(t_mols, nt, t_atoms, t_atom_records, t_bonds, t_bond_records, t_text, t_text_bytes);
    for (const PackedTables* s : {&q, &t})
        if (!s->mols || (!s->atoms && s->n_atom_records) || (!s->bonds && s->n_bond_records) || (!s->text && s->n_text_bytes))
            return bad("null pointer");
    if (!pairs || !recs || !maps) return bad("null pointer");
    if (nq < 1 || nq > 65536 || nt < 1 || nt > 65536) return bad("1 <= nq <= 65536 and 1 <= nt <= 65536 required");
    if (n_pairs < 1 || n_pairs > 1048576) return bad("1 <= n_pairs <= 1048576 required");
    if ((((uintptr_t)q.mols | (uintptr_t)q.atoms | (uintptr_t)q.bonds | (uintptr_t)t.mols | (uintptr_t)t.atoms | (uintptr_t)t.bonds) & 7) ||
        (((uintptr_t)pairs | (uintptr_t)recs) & 3) || ((uintptr_t)maps & 1))
        return bad("mols, atoms and bonds of both sides must be 8-byte aligned, pairs and recs 4-byte, maps 2-byte");
    if (!h->have_st) return bad("call mnx_set_symbol_tables first");
    if (max_matches > 65535) return bad("max_matches must not exceed 65535");
    if (max_steps > MNX_MATCH_MAX_STEPS) return bad("max_steps must not exceed MNX_MATCH_MAX_STEPS (1048576)");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, match_enqueue(h->st_dev, q, t, pairs, n_pairs, recs, maps, max_matches ? max_matches : 1u,
                            max_steps ? max_steps : MNX_MATCH_DEFAULT_STEPS, (hipStream_t)stream));
    return MNX_OK;
}

int mnx_tanimoto(mnx_engine* h, const uint32_t* a, const uint32_t* b, int32_t n, uint32_t* both, uint32_t* either,
                 double* similarity, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const char* m) { h->err = std::string("mnx_tanimoto: ") + m; return MNX_ERR_INVALID_ARG; };
    if (!a || !b) return bad("null pointer");
    if (!both && !either && !similarity) return bad("both, either and similarity are all null");
    if (n < 1 || n > 65536) return bad("1 <= n <= 65536 required");
    if ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)both | (uintptr_t)either) & 3) || ((uintptr_t)similarity & 7))
        return bad("a, b, both and either must be 4-byte aligned, similarity 8-byte");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, tanimoto_enqueue(a, b, n, both, either, similarity, (hipStream_t)stream));
    return MNX_OK;
}

static bool nearest_shape_ok(int32_t nq, uint32_t nl, uint32_t k) {
    return nq >= 1 && nq <= (int32_t)MNX_NEAREST_MAX_QUERIES && nl >= 1 && nl <= MNX_NEAREST_MAX_ROWS && k >= 1 && k <= MNX_NEAREST_MAX_K;
}

size_t mnx_tanimoto_search_work_bytes(int32_t nq, uint32_t nl, uint32_t k) {
    return nearest_shape_ok(nq, nl, k) ? tanimoto_search_work_bytes(nq, nl, k) : 0;
}

int mnx_tanimoto_search(mnx_engine* h, const uint32_t* queries, int32_t nq, const uint32_t* library, uint32_t nl, uint32_t k,
                        double min_similarity, uint32_t flags, uint32_t* count, uint32_t* index, uint32_t* both,
                        uint32_t* either, double* similarity, void* work, size_t work_bytes, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const char* m) { h->err = std::string("mnx_tanimoto_search: ") + m; return MNX_ERR_INVALID_ARG; };
    if (!queries || !library || !count || !index || !work) return bad("null pointer");
    if (nq < 1 || nq > (int32_t)MNX_NEAREST_MAX_QUERIES) return bad("1 <= nq <= 4096 required");
    if (nl < 1 || nl > MNX_NEAREST_MAX_ROWS) return bad("1 <= nl <= 16777216 required");
    if (k < 1 || k > MNX_NEAREST_MAX_K) return bad("1 <= k <= 64 required");
    if (!(min_similarity >= 0.0 && min_similarity <= 1.0)) return bad("0 <= min_similarity <= 1 required");       // a NaN fails both
    if (flags & ~MNX_NEAREST_SKIP_SELF) return bad("flags may hold MNX_NEAREST_SKIP_SELF only");
    if (work_bytes < tanimoto_search_work_bytes(nq, nl, k)) return bad("work_bytes is below mnx_tanimoto_search_work_bytes(nq, nl, k)");
    if ((((uintptr_t)queries | (uintptr_t)library | (uintptr_t)count | (uintptr_t)index | (uintptr_t)both | (uintptr_t)either) & 3) ||
        (((uintptr_t)similarity | (uintptr_t)work) & 7))
        return bad("queries, library, count, index, both and either must be 4-byte aligned, similarity and work 8-byte");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, tanimoto_search_enqueue(queries, nq, library, nl, k, min_similarity, flags, count, index, both, either, similarity, work,
                                      (hipStream_t)stream));
    return MNX_OK;
}

}  // extern "C"
