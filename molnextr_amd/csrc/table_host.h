// table_host.h — the host work of mnx_set_vocab_text, mnx_set_symbol_tables and mnx_set_fragments (engine_tables.hip): the caller's
// arrays validated and laid out as the device reads them (table_types.h). C++17 and no HIP, so that tools/tables_host.cpp runs this
// very text under the host compiler's sanitizers: it walks offsets and records that the caller supplies.
// Each builder returns the empty string and the finished image in *out, or the message its entry point refuses the call with.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "table_types.h"

namespace mnx {

// sym_offset: cfg.sym_offset, the number of symbol ids the vocabulary has
inline std::string build_vocab_text(const char* bytes, const uint32_t* offsets, int32_t n, int32_t sym_offset, VocabText* out) {
    if (!bytes || !offsets || n < 1 || n > 256) return "mnx_set_vocab_text: null pointer or n outside 1..256";
    if (n != sym_offset)      // a shorter table would spell shortened SMILES without a word
        return "mnx_set_vocab_text: n = " + std::to_string(n) + " names, but the vocabulary has cfg.sym_offset = " +
               std::to_string(sym_offset) + " symbol ids";
    if (offsets[0] != 0) return "mnx_set_vocab_text: offsets[0] must be 0";
    VocabText& vt = *out;
    memset(&vt, 0, sizeof(vt));
    for (int i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > 8)
            return "mnx_set_vocab_text: name of id " + std::to_string(i) + " is longer than 8 bytes or its offsets decrease";
        vt.len[i] = (unsigned char)(offsets[i + 1] - offsets[i]);
        memcpy(vt.name[i], bytes + offsets[i], vt.len[i]);
    }
    return "";
}

inline std::string build_symbol_tables(const char* bytes, const uint32_t* offsets, const uint8_t* kinds, int32_t n, SymbolTables* st) {
    auto bad = [&](const std::string& m) { return "mnx_set_symbol_tables: " + m; };
    if (n < 0 || n > 512) return bad("n outside 0..512");
    if (n > 0 && (!bytes || !offsets || !kinds)) return bad("null pointer");
    if (n > 0 && offsets[0] != 0) return bad("offsets[0] must be 0");
    memset(st, 0, sizeof(SymbolTables));
    st->n = n;
    for (int i = 0; i < n; ++i) {
        if (offsets[i + 1] <= offsets[i] || offsets[i + 1] - offsets[i] > 16)
            return bad("name " + std::to_string(i) + " is empty or longer than 16 bytes, or its offsets decrease");
        if (kinds[i] != 1 && kinds[i] != 2) return bad("kinds[" + std::to_string(i) + "] must be 1 (R-group) or 2 (abbreviation)");
        st->len[i] = (unsigned char)(offsets[i + 1] - offsets[i]);
        st->kind[i] = kinds[i];
        memcpy(st->name[i], bytes + offsets[i], st->len[i]);
        if (i > 0) {        // bytewise order, a prefix in front of the longer name: what the device's binary search assumes
            const int m = std::min(st->len[i - 1], st->len[i]), c = memcmp(st->name[i - 1], st->name[i], (size_t)m);
            if (c > 0 || (c == 0 && st->len[i - 1] >= st->len[i]))
                return bad("names must be strictly ascending bytewise; name " + std::to_string(i) + " is not behind its predecessor");
        }
    }
    return "";
}

// the one allocation a FragView points into: frag_of_name | records | atoms | bonds | text begin at off[0 .. 4], each part 8-byte
// aligned (with room for one element where it has none, so that no part is empty)
struct FragImage {
    std::vector<unsigned char> blob;
    size_t off[5];
};

// st_kind, st_n: the kinds and the n of the last mnx_set_symbol_tables, which frag_of_name is parallel to
inline std::string build_fragments(const mnx_mol* frags, int32_t n_frags, const mnx_atom* atoms, uint32_t na, const mnx_bond* bonds,
                                   uint32_t nb, const char* text, uint32_t nt, const int32_t* frag_of_name, int32_t n_names,
                                   const unsigned char* st_kind, int32_t st_n, FragImage* out) {
    auto bad = [&](const std::string& m) { return "mnx_set_fragments: " + m; };
    if (n_frags < 0 || n_frags > 512) return bad("n_frags outside 0..512");
    if (n_names != st_n) return bad("n_names must be the n of mnx_set_symbol_tables (" + std::to_string(st_n) + ")");
    if ((n_frags > 0 && !frags) || (na && !atoms) || (nb && !bonds) || (nt && !text) || (n_names > 0 && !frag_of_name))
        return bad("null pointer");
    // the device copy, put together on the host: bonds sorted by (i, j), every fragment's symbols behind one another
    std::vector<FragRec> rec((size_t)n_frags);
    std::vector<unsigned> fa, fb;
    std::vector<unsigned char> ft;
    for (int f = 0; f < n_frags; ++f) {
        const mnx_mol& m = frags[f];
        const std::string who = "fragment " + std::to_string(f);
        if (m.n_atoms < 1 || m.n_atoms > 32) return bad(who + " has " + std::to_string(m.n_atoms) + " atoms; 1 to 32 required");
        if ((uint64_t)m.atom0 + m.n_atoms > na || (uint64_t)m.bond0 + m.n_bonds > nb || (uint64_t)m.text0 + m.smiles_len > nt)
            return bad(who + ": its records end behind a table");
        FragRec& r = rec[(size_t)f];
        r.atom0 = (unsigned)fa.size(); r.bond0 = (unsigned)fb.size(); r.text0 = (unsigned)ft.size();
        r.n_atoms = (unsigned short)m.n_atoms;
        unsigned len = 0;
        for (uint32_t a = 0; a < m.n_atoms; ++a) {
            const mnx_atom& x = atoms[m.atom0 + a];
            if (x.sym_len < 1 || x.sym_len > 8) return bad(who + ", atom " + std::to_string(a) + ": a symbol has 1 to 8 bytes");
            if ((uint64_t)m.text0 + x.sym0 + x.sym_len > nt) return bad(who + ", atom " + std::to_string(a) + ": its symbol ends behind the text");
            fa.push_back(len | (unsigned)x.sym_len << 16);
            ft.insert(ft.end(), (const unsigned char*)text + m.text0 + x.sym0, (const unsigned char*)text + m.text0 + x.sym0 + x.sym_len);
            len += x.sym_len;
        }
        r.text_len = (unsigned short)len;
        std::vector<unsigned> own;
        for (uint32_t k = 0; k < m.n_bonds; ++k) {
            const mnx_bond& x = bonds[m.bond0 + k];
            const std::string which = who + ", bond " + std::to_string(k);
            if (!(x.i < x.j && x.j < m.n_atoms)) return bad(which + ": i < j < n_atoms required");
            if (x.type < 1 || x.type > 4 || x.rev != x.type) return bad(which + ": type 1 to 4 and rev == type required");
            own.push_back((unsigned)x.i | (unsigned)x.j << 8 | (unsigned)x.type << 16);
        }
        std::sort(own.begin(), own.end(), [](unsigned p, unsigned q) { return ((p & 0xff) << 8 | (p >> 8 & 0xff)) < ((q & 0xff) << 8 | (q >> 8 & 0xff)); });
        unsigned n0 = 0;
        for (size_t k = 0; k < own.size(); ++k) {
            if (k > 0 && (own[k] & 0xffff) == (own[k - 1] & 0xffff)) return bad(who + ": the same pair of atoms in two bonds");
            n0 += (own[k] & 0xff) == 0;
        }
        r.n_bonds = (unsigned short)own.size();
        r.n_bonds0 = (unsigned short)n0;
        fb.insert(fb.end(), own.begin(), own.end());
    }
    for (int k = 0; k < n_names; ++k) {
        if (frag_of_name[k] < -1 || frag_of_name[k] >= n_frags) return bad("frag_of_name[" + std::to_string(k) + "] outside -1.." + std::to_string(n_frags - 1));
        if (frag_of_name[k] >= 0 && st_kind[k] != 2) return bad("frag_of_name[" + std::to_string(k) + "]: only an abbreviation (kind 2) takes a fragment");
    }
    // one allocation: frag_of_name | records | atoms | bonds | text, each part 8-byte aligned
    auto up8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
    const size_t o_rec = up8((size_t)std::max(n_names, 1) * sizeof(int)), o_atoms = o_rec + up8(std::max(rec.size(), (size_t)1) * sizeof(FragRec));
    const size_t o_bonds = o_atoms + up8(std::max(fa.size(), (size_t)1) * 4), o_text = o_bonds + up8(std::max(fb.size(), (size_t)1) * 4);
    const size_t total = o_text + up8(std::max(ft.size(), (size_t)1));
    std::vector<unsigned char>& blob = out->blob;
    blob.assign(total, 0);
    if (n_names) memcpy(blob.data(), frag_of_name, (size_t)n_names * sizeof(int));
    if (!rec.empty()) memcpy(blob.data() + o_rec, rec.data(), rec.size() * sizeof(FragRec));
    if (!fa.empty()) memcpy(blob.data() + o_atoms, fa.data(), fa.size() * 4);
    if (!fb.empty()) memcpy(blob.data() + o_bonds, fb.data(), fb.size() * 4);
    if (!ft.empty()) memcpy(blob.data() + o_text, ft.data(), ft.size());
    out->off[0] = 0; out->off[1] = o_rec; out->off[2] = o_atoms; out->off[3] = o_bonds; out->off[4] = o_text;
    return "";
}

}  // namespace mnx
