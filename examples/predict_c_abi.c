/* examples/predict_c_abi.c — the C ABI used from plain C (no Python, no torch): what a non-Python host of the MolNexTR
 * predict path would write. Builds with:   hipcc -Iinclude examples/predict_c_abi.c -Lmolnextr_amd/lib -lmolnextr_hip
 * (or gcc + -lamdhip64). It only shows the call sequence; weights come from the caller's checkpoint reader. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "molnextr_hip.h"

/* hipMalloc / hipFree prototypes kept local so that the example compiles with a bare C compiler too */
extern int hipMalloc(void** p, size_t n);
extern int hipFree(void* p);
extern int hipMemcpy(void* dst, const void* src, size_t n, int kind);

/* Molecule 0 as a V2000 molfile, written on the device from the tables mnx_graph_pack left there (mnx_molfile_pack): a sizing
 * call without a buffer, then the call that fills it. scale NULL: the reference's factor 10 on a square page. */
static int print_first_molfile(mnx_engine* eng, int n_images, const mnx_mol* mols_dev, const mnx_atom* atoms_dev,
                               const mnx_bond* bonds_dev, const char* text_dev, const uint32_t* table_sizes) {
    uint32_t totals[2] = {0, 0}, *totals_dev = NULL;
    mnx_molfile *files_dev = NULL, file;
    char *out_dev = NULL, *out = NULL;
    int rc, pass;
    hipMalloc((void**)&files_dev, (size_t)n_images * sizeof(mnx_molfile));
    hipMalloc((void**)&totals_dev, sizeof totals);
    for (pass = 0; pass < 2; ++pass) {
        rc = mnx_molfile_pack(eng, mols_dev, n_images, atoms_dev, table_sizes[0], bonds_dev, table_sizes[1], text_dev,
                              table_sizes[2], /*scale=*/NULL, files_dev, out_dev, pass ? totals[0] : 0, totals_dev, /*stream=*/NULL);
        if (rc != MNX_OK) { fprintf(stderr, "mnx_molfile_pack: %s\n", mnx_last_error(eng)); break; }
        hipMemcpy(totals, totals_dev, sizeof totals, 2);
        if (pass == 0 && totals[0]) hipMalloc((void**)&out_dev, totals[0]);
    }
    if (rc == MNX_OK) {
        hipMemcpy(&file, files_dev, sizeof file, 2);
        out = (char*)malloc((size_t)file.len + 1);
        if (out && file.len) {       /* len 0: more than 999 atoms or bonds (MNX_MOLFILE_TOO_LARGE), or records beyond the tables */
            hipMemcpy(out, out_dev + file.text0, file.len, 2);
            printf("molfile 0 (%u bytes%s):\n%.*s", (unsigned)file.len,
                   (file.flags & MNX_MOLFILE_PSEUDO_ATOM) ? ", with R-groups / abbreviations as pseudo-atoms" : "", (int)file.len, out);
        }
        free(out);
    }
    hipFree(files_dev); hipFree(totals_dev); hipFree(out_dev);
    return rc;
}

/* Molecule 0 as a SMILES of the predicted graph, written on the device from the same tables (mnx_smiles_pack_marks with both
 * kinds of marks; the plain mnx_smiles_pack takes the same arguments without `marks` and writes the same string without '@',
 * '/' and '\'): the token SMILES printed above names the atoms, this one joins them with the bonds of the bond head, marks the
 * carbons at which a wedge begins with '@' / '@@' and the double bonds off every cycle with '/' and '\' after the drawing.
 * Valid, not canonical; R-groups and abbreviations stay '*'. The same two passes; `order` (each atom's position in the
 * string) is not asked for here. */
static int print_first_graph_smiles(mnx_engine* eng, int n_images, const mnx_mol* mols_dev, const mnx_atom* atoms_dev,
                                    const mnx_bond* bonds_dev, const char* text_dev, const uint32_t* table_sizes) {
    uint32_t totals[2] = {0, 0}, *totals_dev = NULL;
    mnx_smiles *recs_dev = NULL, rec;
    char *out_dev = NULL, *out = NULL;
    int rc, pass;
    hipMalloc((void**)&recs_dev, (size_t)n_images * sizeof(mnx_smiles));
    hipMalloc((void**)&totals_dev, sizeof totals);
    for (pass = 0; pass < 2; ++pass) {
        rc = mnx_smiles_pack_marks(eng, mols_dev, n_images, atoms_dev, table_sizes[0], bonds_dev, table_sizes[1], text_dev,
                                   table_sizes[2], recs_dev, /*order=*/NULL, out_dev, pass ? totals[0] : 0, totals_dev,
                                   MNX_SMILES_MARK_TETRAHEDRAL | MNX_SMILES_MARK_DOUBLE_BOND, /*stream=*/NULL);
        if (rc != MNX_OK) { fprintf(stderr, "%s\n", mnx_last_error(eng)); break; }
        hipMemcpy(totals, totals_dev, sizeof totals, 2);
        if (pass == 0 && totals[0]) hipMalloc((void**)&out_dev, totals[0]);
    }
    if (rc == MNX_OK) {
        hipMemcpy(&rec, recs_dev, sizeof rec, 2);
        out = (char*)malloc((size_t)rec.len + 1);
        if (rec.flags & (MNX_SMILES_TOO_LARGE | MNX_SMILES_BEYOND_TABLES | MNX_SMILES_DUPLICATE_BOND | MNX_SMILES_RING_NUMBERS)) {
            printf("graph SMILES 0: none (flags 0x%x)\n", (unsigned)rec.flags);
        } else if (out) {
            if (rec.len) hipMemcpy(out, out_dev + rec.text0, rec.len, 2);
            printf("graph SMILES 0: %.*s (%u ring bonds%s%s%s%s%s%s)\n", (int)rec.len, out, (unsigned)rec.n_rings,
                   (rec.flags & MNX_SMILES_STEREO) ? ", stereo marks" : "",
                   (rec.flags & MNX_SMILES_STEREO_UNRESOLVED) ? ", a marked carbon unresolved" : "",
                   (rec.flags & MNX_SMILES_EZ) ? ", double-bond marks" : "",
                   (rec.flags & MNX_SMILES_EZ_UNRESOLVED) ? ", a double bond unresolved" : "",
                   (rec.flags & MNX_SMILES_EZ_IMPLIED) ? ", a configuration implied" : "",
                   (rec.flags & MNX_SMILES_WEDGES_DROPPED) ? ", wedges dropped" : "");
        }
        free(out);
    }
    hipFree(recs_dev); hipFree(totals_dev); hipFree(out_dev);
    return rc;
}

/* Molecule 0 once more, on canonical atom ranks (mnx_smiles_pack_canonical, here without marks): the bytes no longer depend on
 * the order in which the decoder emitted the atoms, so a host without a toolkit can compare, count and cache them. `rank` is
 * required (it carries the ranks from the first launch to the others), `sym_class` and `order` are optional. This library's
 * own ranking: NOT RDKit's canonical SMILES, and the header names the few graphs whose string still depends on the drawing. */
static int print_first_canonical_smiles(mnx_engine* eng, int n_images, const mnx_mol* mols_dev, const mnx_atom* atoms_dev,
                                        const mnx_bond* bonds_dev, const char* text_dev, const uint32_t* table_sizes) {
    uint32_t totals[2] = {0, 0}, *totals_dev = NULL;
    uint16_t* rank_dev = NULL;
    mnx_smiles *recs_dev = NULL, rec;
    char *out_dev = NULL, *out = NULL;
    int rc, pass;
    hipMalloc((void**)&recs_dev, (size_t)n_images * sizeof(mnx_smiles));
    hipMalloc((void**)&totals_dev, sizeof totals);
    hipMalloc((void**)&rank_dev, ((size_t)table_sizes[0] + 1) * sizeof(uint16_t));
    for (pass = 0; pass < 2; ++pass) {
        rc = mnx_smiles_pack_canonical(eng, mols_dev, n_images, atoms_dev, table_sizes[0], bonds_dev, table_sizes[1], text_dev,
                                       table_sizes[2], recs_dev, /*order=*/NULL, rank_dev, /*sym_class=*/NULL, out_dev,
                                       pass ? totals[0] : 0, totals_dev, /*marks=*/0, /*stream=*/NULL);
        if (rc != MNX_OK) { fprintf(stderr, "%s\n", mnx_last_error(eng)); break; }
        hipMemcpy(totals, totals_dev, sizeof totals, 2);
        if (pass == 0 && totals[0]) hipMalloc((void**)&out_dev, totals[0]);
    }
    if (rc == MNX_OK) {
        hipMemcpy(&rec, recs_dev, sizeof rec, 2);
        out = (char*)malloc((size_t)rec.len + 1);
        if (rec.flags & (MNX_SMILES_TOO_LARGE | MNX_SMILES_BEYOND_TABLES | MNX_SMILES_DUPLICATE_BOND | MNX_SMILES_RING_NUMBERS)) {
            printf("canonical graph SMILES 0: none (flags 0x%x)\n", (unsigned)rec.flags);
        } else if (out) {
            if (rec.len) hipMemcpy(out, out_dev + rec.text0, rec.len, 2);
            printf("canonical graph SMILES 0: %.*s%s%s\n", (int)rec.len, out,
                   (rec.flags & MNX_SMILES_CANON_TIE) ? " (a tie broken by the drawing)" : "",
                   (rec.flags & MNX_SMILES_CANON_TIE_INDEX) ? " (and one by the atom index)" : "");
        }
        free(out);
    }
    hipFree(recs_dev); hipFree(totals_dev); hipFree(rank_dev); hipFree(out_dev);
    return rc;
}

/* The same molecules with their abbreviation labels ('Ph', 'OMe', 'Boc', ...) replaced by atoms and bonds (mnx_expand_pack), and
 * molecule 0's canonical SMILES written from THOSE tables: packed tables in, packed tables of the same record types out, so the
 * writers above take them as they are. A sizing call with capacities 0 (`totals` is complete whatever the capacities), then
 * the call itself. From a table only (a label without a fragment stays a '*'), the atoms of a fragment share the label's
 * coordinates, and no toolkit has parsed the result. */
static int print_first_expanded_smiles(mnx_engine* eng, int n_images, const mnx_mol* mols_dev, const mnx_atom* atoms_dev,
                                       const mnx_bond* bonds_dev, const char* text_dev, const uint32_t* table_sizes) {
    uint32_t totals[4] = {0, 0, 0, 0}, *totals_dev = NULL;
    mnx_mol *mols2_dev = NULL, mol;
    mnx_atom* atoms2_dev = NULL;
    mnx_bond* bonds2_dev = NULL;
    char* text2_dev = NULL;
    int rc, pass;
    hipMalloc((void**)&mols2_dev, (size_t)n_images * sizeof(mnx_mol));
    hipMalloc((void**)&totals_dev, sizeof totals);
    for (pass = 0; pass < 2; ++pass) {
        rc = mnx_expand_pack(eng, mols_dev, n_images, atoms_dev, table_sizes[0], bonds_dev, table_sizes[1], text_dev, table_sizes[2],
                             mols2_dev, atoms2_dev, pass ? totals[0] : 0, bonds2_dev, pass ? totals[1] : 0, text2_dev,
                             pass ? totals[2] : 0, /*origin=*/NULL, totals_dev, /*stream=*/NULL);
        if (rc != MNX_OK) { fprintf(stderr, "%s\n", mnx_last_error(eng)); break; }
        hipMemcpy(totals, totals_dev, sizeof totals, 2);
        if (pass == 0) {
            hipMalloc((void**)&atoms2_dev, ((size_t)totals[0] + 1) * sizeof(mnx_atom));
            hipMalloc((void**)&bonds2_dev, ((size_t)totals[1] + 1) * sizeof(mnx_bond));
            hipMalloc((void**)&text2_dev, (size_t)totals[2] + 1);
        }
    }
    if (rc == MNX_OK) {
        hipMemcpy(&mol, mols2_dev, sizeof mol, 2);
        printf("molecule 0 expanded: %u atoms, %u bonds%s%s%s\n", (unsigned)mol.n_atoms, (unsigned)mol.n_bonds,
               (mol.flags & MNX_MOL_EXPANDED) ? ", a label replaced" : "", (mol.flags & MNX_MOL_LABEL_LEFT) ? ", a label left" : "",
               (mol.flags & MNX_MOL_EXPAND_REFUSED) ? ", refused" : "");
        rc = print_first_canonical_smiles(eng, n_images, mols2_dev, atoms2_dev, bonds2_dev, text2_dev, totals);
    }
    if (rc == MNX_OK) {     /* behind the expansion: only the largest connected component (mnx_main_pack, the reference's
                             * --keep_main_molecule). Nothing grows, so tables of the input's sizes always suffice. */
        mnx_mol* mols3_dev = NULL;
        mnx_atom* atoms3_dev = NULL;
        mnx_bond* bonds3_dev = NULL;
        char* text3_dev = NULL;
        hipMalloc((void**)&mols3_dev, (size_t)n_images * sizeof(mnx_mol));
        hipMalloc((void**)&atoms3_dev, ((size_t)totals[0] + 1) * sizeof(mnx_atom));
        hipMalloc((void**)&bonds3_dev, ((size_t)totals[1] + 1) * sizeof(mnx_bond));
        hipMalloc((void**)&text3_dev, (size_t)totals[2] + 1);
        rc = mnx_main_pack(eng, mols2_dev, n_images, atoms2_dev, totals[0], bonds2_dev, totals[1], text2_dev, totals[2], mols3_dev,
                           atoms3_dev, totals[0], bonds3_dev, totals[1], text3_dev, totals[2], /*origin=*/NULL, totals_dev, /*stream=*/NULL);
        if (rc != MNX_OK) fprintf(stderr, "%s\n", mnx_last_error(eng));
        else {
            hipMemcpy(totals, totals_dev, sizeof totals, 2);
            hipMemcpy(&mol, mols3_dev, sizeof mol, 2);
            printf("molecule 0, main component: %u atoms%s%s\n", (unsigned)mol.n_atoms, (mol.flags & MNX_MOL_MAIN_KEPT) ? ", atoms dropped" : "",
                   (mol.flags & MNX_MOL_MAIN_TIE) ? ", a tie" : "");
            rc = print_first_canonical_smiles(eng, n_images, mols3_dev, atoms3_dev, bonds3_dev, text3_dev, totals);
        }
        if (rc == MNX_OK) {     /* behind the chain: the path fingerprint of every main molecule (mnx_fingerprint_pack, this library's
                                 * own rule, not RDKit's bits) and how similar molecule 0 is to the last one (mnx_tanimoto) */
            mnx_fp* fp_dev = NULL, fp;
            uint32_t *bits_dev = NULL, both = 0, *both_dev = NULL;
            double similarity = 0.0, *similarity_dev = NULL;
            hipMalloc((void**)&fp_dev, (size_t)n_images * sizeof(mnx_fp));
            hipMalloc((void**)&bits_dev, (size_t)n_images * MNX_FP_WORDS * sizeof(uint32_t));
            hipMalloc((void**)&both_dev, sizeof both);
            hipMalloc((void**)&similarity_dev, sizeof similarity);
            rc = mnx_fingerprint_pack(eng, mols3_dev, n_images, atoms3_dev, totals[0], bonds3_dev, totals[1], text3_dev, totals[2], fp_dev,
                                      bits_dev, /*max_bonds=*/0, /*max_steps=*/0, /*stream=*/NULL);
            if (rc == MNX_OK)
                rc = mnx_tanimoto(eng, bits_dev, bits_dev + (size_t)(n_images - 1) * MNX_FP_WORDS, 1, both_dev, /*either=*/NULL,
                                  similarity_dev, /*stream=*/NULL);
            if (rc != MNX_OK) fprintf(stderr, "%s\n", mnx_last_error(eng));
            else {
                hipMemcpy(&fp, fp_dev, sizeof fp, 2);
                hipMemcpy(&both, both_dev, sizeof both, 2);
                hipMemcpy(&similarity, similarity_dev, sizeof similarity, 2);
                printf("molecule 0, fingerprint: %u bits%s, %u shared with molecule %d, Tanimoto %.3f\n", (unsigned)fp.n_bits,
                       (fp.flags & MNX_FP_LIMIT) ? " (step limit)" : "", (unsigned)both, n_images - 1, similarity);
            }
            hipFree(fp_dev); hipFree(bits_dev); hipFree(both_dev); hipFree(similarity_dev);
        }
        hipFree(mols3_dev); hipFree(atoms3_dev); hipFree(bonds3_dev); hipFree(text3_dev);
    }
    hipFree(mols2_dev); hipFree(totals_dev); hipFree(atoms2_dev); hipFree(bonds2_dev); hipFree(text2_dev);
    return rc;
}

/* The same molecules with their condensed-formula labels ('CH2CH3', 'N(CH3)2', 'COOCH3', 'CH2Ph': labels that are in neither
 * name table) replaced by the atoms and bonds a valence-guided search finds for them (mnx_formula_pack), in front of the
 * expansion above, which also replaces the group tokens a formula holds ('[Ph]'): the same two passes of sizing and writing. The
 * rule is this library's own repair of the reference's search; no toolkit has parsed the result, and a label the search finds
 * no structure for stays a '*'. */
static int print_first_formula_smiles(mnx_engine* eng, int n_images, const mnx_mol* mols_dev, const mnx_atom* atoms_dev,
                                      const mnx_bond* bonds_dev, const char* text_dev, const uint32_t* table_sizes) {
    uint32_t totals[4] = {0, 0, 0, 0}, *totals_dev = NULL;
    mnx_mol *mols2_dev = NULL, mol;
    mnx_atom* atoms2_dev = NULL;
    mnx_bond* bonds2_dev = NULL;
    char* text2_dev = NULL;
    int rc, pass;
    hipMalloc((void**)&mols2_dev, (size_t)n_images * sizeof(mnx_mol));
    hipMalloc((void**)&totals_dev, sizeof totals);
    for (pass = 0; pass < 2; ++pass) {
        rc = mnx_formula_pack(eng, mols_dev, n_images, atoms_dev, table_sizes[0], bonds_dev, table_sizes[1], text_dev, table_sizes[2],
                              mols2_dev, atoms2_dev, pass ? totals[0] : 0, bonds2_dev, pass ? totals[1] : 0, text2_dev,
                              pass ? totals[2] : 0, /*origin=*/NULL, totals_dev, /*max_steps=*/0, /*stream=*/NULL);
        if (rc != MNX_OK) { fprintf(stderr, "%s\n", mnx_last_error(eng)); break; }
        hipMemcpy(totals, totals_dev, sizeof totals, 2);
        if (pass == 0) {
            hipMalloc((void**)&atoms2_dev, ((size_t)totals[0] + 1) * sizeof(mnx_atom));
            hipMalloc((void**)&bonds2_dev, ((size_t)totals[1] + 1) * sizeof(mnx_bond));
            hipMalloc((void**)&text2_dev, (size_t)totals[2] + 1);
        }
    }
    if (rc == MNX_OK) {
        hipMemcpy(&mol, mols2_dev, sizeof mol, 2);
        printf("molecule 0 with its formulas replaced: %u atoms, %u bonds%s%s%s\n", (unsigned)mol.n_atoms, (unsigned)mol.n_bonds,
               (mol.flags & MNX_MOL_FORMULA_EXPANDED) ? ", a formula replaced" : "", (mol.flags & MNX_MOL_FORMULA_LEFT) ? ", a formula left" : "",
               (mol.flags & MNX_MOL_FORMULA_REFUSED) ? ", refused" : "");
        rc = print_first_expanded_smiles(eng, n_images, mols2_dev, atoms2_dev, bonds2_dev, text2_dev, totals);
    }
    hipFree(mols2_dev); hipFree(totals_dev); hipFree(atoms2_dev); hipFree(bonds2_dev); hipFree(text2_dev);
    return rc;
}

/* A caller's own SMILES in the form the predictions are written in (mnx_smiles_read, then the canonical writer): two strings of
 * one molecule read on the device into packed tables of the same record types, so print_first_canonical_smiles takes them as
 * they are. Needs no symbol tables itself; a refused string (mnx_read.flags) is the empty molecule. No toolkit has parsed these
 * strings: the reader and the writers are each other's check. */
static int print_canonical_of_known_smiles(mnx_engine* eng) {
    static const char known[] = "OCCc1ccccc1CCO";                 /* two strings behind one another: "OCC" and "c1ccccc1CCO" */
    const uint32_t offsets[3] = {0, 3, 14};
    uint32_t totals[4] = {0, 0, 0, 0}, *totals_dev = NULL, *offsets_dev = NULL;
    char *bytes_dev = NULL, *text_dev = NULL;
    mnx_mol* mols_dev = NULL;
    mnx_read *recs_dev = NULL, recs[2];
    mnx_atom* atoms_dev = NULL;
    mnx_bond* bonds_dev = NULL;
    int rc;
    hipMalloc((void**)&bytes_dev, sizeof known); hipMalloc((void**)&offsets_dev, sizeof offsets);
    hipMalloc((void**)&mols_dev, 2 * sizeof(mnx_mol)); hipMalloc((void**)&recs_dev, sizeof recs);
    hipMalloc((void**)&atoms_dev, 14 * sizeof(mnx_atom)); hipMalloc((void**)&bonds_dev, 14 * sizeof(mnx_bond));   /* an atom and a */
    hipMalloc((void**)&text_dev, 14); hipMalloc((void**)&totals_dev, sizeof totals);                               /* bond per byte */
    hipMemcpy(bytes_dev, known, 14, 1 /* hipMemcpyHostToDevice */);
    hipMemcpy(offsets_dev, offsets, sizeof offsets, 1);
    rc = mnx_smiles_read(eng, bytes_dev, 14, offsets_dev, 2, mols_dev, recs_dev, atoms_dev, 14, bonds_dev, 14, text_dev, 14,
                         totals_dev, /*stream=*/NULL);
    if (rc != MNX_OK) fprintf(stderr, "%s\n", mnx_last_error(eng));
    else {
        hipMemcpy(totals, totals_dev, sizeof totals, 2);
        hipMemcpy(recs, recs_dev, sizeof recs, 2);
        if (recs[0].flags & MNX_READ_SYNTAX) printf("string 0: a rule of the grammar breaks at byte %u\n", (unsigned)recs[0].err_pos);
        rc = print_first_canonical_smiles(eng, 2, mols_dev, atoms_dev, bonds_dev, text_dev, totals);
    }
    hipFree(bytes_dev); hipFree(offsets_dev); hipFree(mols_dev); hipFree(recs_dev); hipFree(atoms_dev); hipFree(bonds_dev);
    hipFree(text_dev); hipFree(totals_dev);
    return rc;
}

/* The molecules as packed tables (mnx_graph_pack): no tokenizer on the host. A first call with modest capacities; `totals`
 * says what the job needs, so a second call with exactly that is the worst case. Prints molecule 0 with its token SMILES, then its molfile and its graph SMILES. */
static int print_first_molecule(mnx_engine* eng, int n_images, const int32_t* tokens, const int32_t* lengths,
                                const int32_t* atom_idx, const int32_t* n_atoms, const uint8_t* edges) {
    uint32_t caps[3], totals[4] = {0, 0, 0, 0}, *totals_dev = NULL, k;
    mnx_mol *mols_dev = NULL, mol;
    mnx_atom *atoms_dev = NULL, *atoms = NULL;
    mnx_bond *bonds_dev = NULL, *bonds = NULL;
    char *text_dev = NULL, *text = NULL;
    int rc = MNX_OK, attempt;
    caps[0] = (uint32_t)n_images * 48; caps[1] = (uint32_t)n_images * 56; caps[2] = (uint32_t)n_images * 192;
    hipMalloc((void**)&mols_dev, (size_t)n_images * sizeof(mnx_mol));
    hipMalloc((void**)&totals_dev, sizeof totals);
    for (attempt = 0; attempt < 2 && rc == MNX_OK; ++attempt) {
        hipMalloc((void**)&atoms_dev, (size_t)caps[0] * sizeof(mnx_atom));
        hipMalloc((void**)&bonds_dev, (size_t)caps[1] * sizeof(mnx_bond));
        hipMalloc((void**)&text_dev, caps[2]);
        /* no confidences here: the three score pointers NULL (mnx_predict_confidence's outputs would go in their place) */
        rc = mnx_graph_pack(eng, tokens, lengths, n_images, 480, atom_idx, n_atoms, edges, 160, NULL, NULL, NULL, mols_dev,
                            atoms_dev, caps[0], bonds_dev, caps[1], text_dev, caps[2], totals_dev, /*stream=*/NULL);
        if (rc != MNX_OK) { fprintf(stderr, "mnx_graph_pack: %s\n", mnx_last_error(eng)); break; }
        hipMemcpy(totals, totals_dev, sizeof totals, 2 /* hipMemcpyDeviceToHost: waits for the three launches */);
        if (!totals[3]) break;
        hipFree(atoms_dev); hipFree(bonds_dev); hipFree(text_dev);
        atoms_dev = NULL; bonds_dev = NULL; text_dev = NULL;
        caps[0] = totals[0]; caps[1] = totals[1]; caps[2] = totals[2];
    }
    if (rc == MNX_OK && !totals[3]) {
        hipMemcpy(&mol, mols_dev, sizeof mol, 2);
        atoms = (mnx_atom*)malloc((size_t)(mol.n_atoms + 1) * sizeof(mnx_atom));
        bonds = (mnx_bond*)malloc((size_t)(mol.n_bonds + 1) * sizeof(mnx_bond));
        text = (char*)malloc((size_t)mol.smiles_len + 1);
        if (atoms && bonds && text) {
            hipMemcpy(atoms, atoms_dev + mol.atom0, (size_t)mol.n_atoms * sizeof(mnx_atom), 2);
            hipMemcpy(bonds, bonds_dev + mol.bond0, (size_t)mol.n_bonds * sizeof(mnx_bond), 2);
            hipMemcpy(text, text_dev + mol.text0, mol.smiles_len, 2);
            printf("molecule 0: %.*s%s\n", (int)mol.smiles_len, text, (mol.flags & MNX_MOL_TRUNCATED) ? " (atoms truncated)" : "");
            for (k = 0; k < mol.n_atoms; ++k)      /* the symbol is a substring of the SMILES; coordinate = bin / (bins - 1) */
                printf("  atom %u  %.*s  (%.3f, %.3f)\n", (unsigned)k, (int)atoms[k].sym_len, text + atoms[k].sym0,
                       atoms[k].x_bin / 63.0, atoms[k].y_bin / 63.0);
            for (k = 0; k < mol.n_bonds; ++k)
                printf("  bond %u - %u  type %u\n", (unsigned)bonds[k].i, (unsigned)bonds[k].j, (unsigned)bonds[k].type);
        }
        free(atoms); free(bonds); free(text);
        rc = print_first_molfile(eng, n_images, mols_dev, atoms_dev, bonds_dev, text_dev, totals);
        if (rc == MNX_OK) rc = print_first_graph_smiles(eng, n_images, mols_dev, atoms_dev, bonds_dev, text_dev, totals);
        if (rc == MNX_OK) rc = print_first_canonical_smiles(eng, n_images, mols_dev, atoms_dev, bonds_dev, text_dev, totals);
        if (rc == MNX_OK) rc = print_first_expanded_smiles(eng, n_images, mols_dev, atoms_dev, bonds_dev, text_dev, totals);
        if (rc == MNX_OK) rc = print_first_formula_smiles(eng, n_images, mols_dev, atoms_dev, bonds_dev, text_dev, totals);
        if (rc == MNX_OK) rc = print_canonical_of_known_smiles(eng);
    }
    hipFree(mols_dev); hipFree(totals_dev); hipFree(atoms_dev); hipFree(bonds_dev); hipFree(text_dev);
    return rc;
}

int run(const mnx_weight_desc* weights, int n_weights, const float* host_images /* [n,3,384,384] */, int n_images) {
    mnx_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.img_size = 384; cfg.patch = 4; cfg.embed_dim = 128; cfg.n_stages = 4; cfg.window = 12;
    { const int d[4] = {2, 2, 18, 2}, h[4] = {4, 8, 16, 32}; memcpy(cfg.depths, d, sizeof d); memcpy(cfg.heads, h, sizeof h); }
    cfg.dec_layers = 6; cfg.dec_dim = 256; cfg.dec_heads = 8; cfg.dec_ff = 1024;
    cfg.vocab = 229; cfg.sym_offset = 101; cfg.coord_bins = 64; cfg.pe_len = 5000;
    cfg.max_len = 480; cfg.max_batch = 64; cfg.max_atoms = 160; cfg.compute_dtype = MNX_DTYPE_FP16X3; cfg.dec_slots = 3072;

    mnx_engine* eng = NULL;
    if (mnx_create(&cfg, weights, n_weights, /*device=*/0, &eng) != MNX_OK) {
        fprintf(stderr, "mnx_create: %s\n", mnx_last_error(NULL));
        return 1;
    }
    /* token classes of the vocabulary (CharTokenizer.is_symbol / is_atom) — see molnextr_amd/engine.py for the table */
    /* mnx_set_token_classes(eng, flags, 101, id_lbracket, id_rbracket, id_C, id_l, id_B, id_r); */
    /* ... and the names of its 101 symbol ids as UTF-8 bytes, for mnx_graph_pack (vocab/vocab_chars.json in id order): */
    /* mnx_set_vocab_text(eng, name_bytes, name_offsets, 101); */
    /* ... and, for mnx_molfile_pack and mnx_smiles_pack, the R-group and abbreviation names sorted bytewise
     * (vocab/abbreviations.json); without this call the molfile step below is refused ("mnx_molfile_pack: call
     * mnx_set_symbol_tables first") and run() fails: */
    /* mnx_set_symbol_tables(eng, table_bytes, table_offsets, table_kinds, n_names); */
    /* ... and, for mnx_expand_pack, the fragments the abbreviation names stand for, as packed tables, with the fragment of every
     * name of the call above or -1 (vocab/fragments.json through molnextr_amd/fragments.py): */
    /* mnx_set_fragments(eng, frags, n_frags, frag_atoms, n_frag_atoms, frag_bonds, n_frag_bonds, frag_text, n_frag_text,
     *                   frag_of_name, n_names); */

    const size_t img_elems = (size_t)3 * 384 * 384;
    float* images = NULL;
    int32_t *tokens = NULL, *lengths = NULL, *n_atoms = NULL, *atom_idx = NULL;
    uint8_t* edges = NULL;
    hipMalloc((void**)&images, n_images * img_elems * sizeof(float));
    hipMalloc((void**)&tokens, (size_t)n_images * 480 * 4);
    hipMalloc((void**)&lengths, (size_t)n_images * 4);
    hipMalloc((void**)&n_atoms, (size_t)n_images * 4);
    hipMalloc((void**)&atom_idx, (size_t)n_images * 160 * 4);
    hipMalloc((void**)&edges, (size_t)n_images * 160 * 160);
    hipMemcpy(images, host_images, n_images * img_elems * sizeof(float), 1 /* hipMemcpyHostToDevice */);

    /* reference batches of 16 images, as `predict_images(batch_size=16)` numbers them (MolNexTR/model.py:97) */
    int rc = mnx_predict(eng, images, n_images, /*ref_batch=*/16, /*max_len=*/480, /*stop_on_eos=*/1, tokens, lengths, n_atoms,
                         atom_idx,
                         edges, /*kmax=*/160, /*stream=*/NULL);
    if (rc != MNX_OK) fprintf(stderr, "mnx_predict: %s\n", mnx_last_error(eng));
    if (rc == MNX_OK) rc = print_first_molecule(eng, n_images, tokens, lengths, atom_idx, n_atoms, edges);

    hipFree(images); hipFree(tokens); hipFree(lengths); hipFree(n_atoms); hipFree(atom_idx); hipFree(edges);
    mnx_destroy(eng);
    return rc != MNX_OK;
}

/* The same from raw pages (HWC uint8 RGB, every page its own size): all pages transformed by ONE mnx_preprocess_batch call
 * into gray bytes, which mnx_predict_gray8 reads directly — a twelfth of the bytes of the fp32 images above, the same results
 * bit for bit. `eng` as created in run(); n_pages <= MNX_PREP_MAX_PAGES per call. */
int run_from_pages(mnx_engine* eng, const uint8_t* const* host_pages, const int32_t* heights, const int32_t* widths,
                   int n_pages) {
    mnx_page* table = (mnx_page*)malloc((size_t)n_pages * sizeof(mnx_page));
    uint64_t arena_bytes = 0;
    int32_t tallest = 1;
    int i, rc;
    uint8_t *arena = NULL, *gray = NULL, *edges = NULL;
    mnx_page* table_dev = NULL;
    int32_t *tokens = NULL, *lengths = NULL, *n_atoms = NULL, *atom_idx = NULL;
    if (!table) return 1;
    for (i = 0; i < n_pages; ++i) {          /* pages side by side in one arena, each at a multiple of 16 bytes */
        table[i].offset = arena_bytes;
        table[i].height = heights[i];
        table[i].width = widths[i];
        arena_bytes += ((uint64_t)3 * (uint64_t)heights[i] * (uint64_t)widths[i] + 15u) & ~(uint64_t)15;
        if (heights[i] > tallest) tallest = heights[i];
    }
    hipMalloc((void**)&arena, (size_t)arena_bytes);
    hipMalloc((void**)&table_dev, (size_t)n_pages * sizeof(mnx_page));
    hipMalloc((void**)&gray, (size_t)n_pages * 384 * 384);
    hipMalloc((void**)&tokens, (size_t)n_pages * 480 * 4);
    hipMalloc((void**)&lengths, (size_t)n_pages * 4);
    hipMalloc((void**)&n_atoms, (size_t)n_pages * 4);
    hipMalloc((void**)&atom_idx, (size_t)n_pages * 160 * 4);
    hipMalloc((void**)&edges, (size_t)n_pages * 160 * 160);
    for (i = 0; i < n_pages; ++i)            /* (a real host stages the pages in ONE pinned buffer and copies once) */
        hipMemcpy(arena + table[i].offset, host_pages[i], (size_t)3 * (size_t)heights[i] * (size_t)widths[i], 1);
    hipMemcpy(table_dev, table, (size_t)n_pages * sizeof(mnx_page), 1 /* hipMemcpyHostToDevice */);

    rc = mnx_preprocess_batch(eng, arena, table_dev, n_pages, tallest, /*pad=*/50, /*pad_to_square=*/0, /*crops_out=*/NULL,
                              gray, MNX_IMG_GRAY8, /*stream=*/NULL);
    if (rc != MNX_OK) fprintf(stderr, "mnx_preprocess_batch: %s\n", mnx_last_error(eng));
    /* the four confidence pointers all NULL: mnx_predict's outputs; all four set: mnx_predict_confidence's */
    if (rc == MNX_OK) {
        rc = mnx_predict_gray8(eng, gray, n_pages, /*ref_batch=*/16, /*max_len=*/480, tokens, lengths, n_atoms, atom_idx, edges,
                               /*kmax=*/160, NULL, NULL, NULL, NULL, /*stream=*/NULL);
        if (rc != MNX_OK) fprintf(stderr, "mnx_predict_gray8: %s\n", mnx_last_error(eng));
    }
    hipFree(arena); hipFree(table_dev); hipFree(gray); hipFree(tokens); hipFree(lengths); hipFree(n_atoms); hipFree(atom_idx);
    hipFree(edges);
    free(table);
    return rc != MNX_OK;
}
