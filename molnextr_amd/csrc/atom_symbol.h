// atom_symbol.h — what the molfile writer (molfile.hip) and the SMILES writer (smiles.hip) do alike before their own work: one
// atom's symbol read as the reference's _convert_graph_to_smiles reads it (chemical.py:886-903: brackets stripped, R-group table,
// abbreviation table, and only then the whole symbol through the bracket-atom grammar), and behind it the admission of one molecule
// of the packed tables and the loop over its atoms. One definition, so the two cannot drift apart (internal). What the writers
// decide differently stays in their kernels: the bond loops, and with them a bond from an atom to itself. This is the INPUT side
// of the post-passes (PackedTables); the output side of those that write tables again (TablesOut) is tables_out.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/molnextr_hip.h"
#include "table_types.h"

namespace mnx {

constexpr int SYM_ALIAS = 70;            // bytes of an alias line of a molfile: the most an interpretation keeps of a pseudo-atom's name

// ---- one atom's interpretation, packed into a word of LDS ----
//   bits 0-1 class: 0 atom of the SMILES grammar, 1 pseudo-atom 'R', 2 numbered R-group 'R#'
//   bit 2 bracket atom, bit 3 one of the four chiral carbon symbols, bits 4-7 H count, bits 8-12 charge + 15,
//   bits 13-22 isotope (class 0) or R-group number (class 2), bits 23-29 alias bytes, bit 30 alias starts behind a '[',
//   bit 31 (class 0) the element is spelled in lower case: an aromatic atom
constexpr unsigned CLS_ATOM = 0, CLS_PSEUDO = 1, CLS_RNUM = 2;
__device__ __forceinline__ unsigned info_cls(unsigned w) { return w & 3u; }
__device__ __forceinline__ int info_h(unsigned w) { return (int)(w >> 4 & 15u); }
__device__ __forceinline__ int info_charge(unsigned w) { return (int)(w >> 8 & 31u) - 15; }
__device__ __forceinline__ unsigned info_num(unsigned w) { return w >> 13 & 1023u; }
__device__ __forceinline__ unsigned info_alias(unsigned w) { return w >> 23 & 127u; }
__device__ __forceinline__ bool info_aromatic(unsigned w) { return (w >> 31) != 0; }

// the 118 element symbols, two bytes each (a one-letter symbol is followed by a blank)
static __device__ const char ELEMENTS[] =
    "H HeLiBeB C N O F NeNaMgAlSiP S ClArK CaScTiV CrMnFeCoNiCuZnGaGeAsSeBrKrRbSrY ZrNbMoTcRuRhPdAgCdInSnSbTeI XeCsBaLaCePrNdPm"
    "SmEuGdTbDyHoErTmYbLuHfTaW ReOsIrPtAuHgTlPbBiPoAtRnFrRaAcThPaU NpPuAmCmBkCfEsFmMdNoLrRfDbSgBhHsMtDsRgCnNhFlMcLvTsOg";
static_assert(sizeof(ELEMENTS) == 2 * 118 + 1, "118 elements");

__device__ __forceinline__ bool is_element(unsigned char a, unsigned char b) {
    for (int i = 0; i < 118; ++i)
        if (ELEMENTS[2 * i] == (char)a && ELEMENTS[2 * i + 1] == (char)b) return true;
    return false;
}
__device__ __forceinline__ bool is_digit(unsigned char c) { return c >= '0' && c <= '9'; }
__device__ __forceinline__ bool is_organic_aromatic(unsigned char c) {
    return c == 'b' || c == 'c' || c == 'n' || c == 'o' || c == 'p' || c == 's';
}

// index of the n bytes at s in the sorted name table, -1 when absent (binary search, bytewise order)
__device__ __forceinline__ int table_find(const SymbolTables* __restrict__ st, const unsigned char* s, int n) {
    if (n < 1 || n > 16) return -1;
    int lo = 0, hi = st->n - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1, ml = st->len[mid];
        int c = 0;
        for (int k = 0; k < min(n, ml) && c == 0; ++k) c = (int)s[k] - (int)st->name[mid][k];
        if (c == 0) c = n - ml;
        if (c == 0) return mid;
        if (c < 0) hi = mid - 1; else lo = mid + 1;
    }
    return -1;
}

// The whole symbol as a SMILES atom (what Chem.AtomFromSmiles takes of the vocabulary's atoms, chemical.py:898): sets the
// element's two bytes (capitalised; 'R' for '*'), whether it was spelled in lower case, H count, charge, isotope; false = no
// parse.
__device__ __forceinline__ bool parse_smiles_atom(const unsigned char* s, int n, unsigned char* e0, unsigned char* e1, bool* lower,
                                                  int* hcount, int* charge, int* isotope) {
    *e1 = ' '; *lower = false; *hcount = 0; *charge = 0; *isotope = 0;
    if (n < 1) return false;
    if (s[0] != '[') {
        const unsigned char c = s[0];
        if (n == 1) {
            if (c == 'B' || c == 'C' || c == 'N' || c == 'O' || c == 'P' || c == 'S' || c == 'F' || c == 'I') { *e0 = c; return true; }
            if (is_organic_aromatic(c)) { *e0 = c - 32; *lower = true; return true; }
            if (c == '*') { *e0 = 'R'; return true; }
            return false;
        }
        if (n == 2 && ((c == 'C' && s[1] == 'l') || (c == 'B' && s[1] == 'r'))) { *e0 = c; *e1 = s[1]; return true; }
        return false;
    }
    if (n < 3 || s[n - 1] != ']') return false;
    const int e = n - 1;
    int p = 1, iso = 0;
    while (p < e && is_digit(s[p])) {
        iso = iso * 10 + (s[p] - '0');
        if (iso > 999) return false;
        ++p;
    }
    if (p >= e) return false;
    const unsigned char c = s[p], d = p + 1 < e ? s[p + 1] : 0;
    if (c == '*') { *e0 = 'R'; ++p; }
    else if ((c == 's' && d == 'e') || (c == 'a' && d == 's')) { *e0 = c - 32; *e1 = d; *lower = true; p += 2; }
    else if (is_organic_aromatic(c)) { *e0 = c - 32; *lower = true; ++p; }
    else if (c >= 'A' && c <= 'Z') {
        if (d >= 'a' && d <= 'z' && is_element(c, d)) { *e0 = c; *e1 = d; p += 2; }      // the longest match wins
        else if (is_element(c, ' ')) { *e0 = c; ++p; }
        else return false;
    } else return false;
    if (p < e && s[p] == '@') { ++p; if (p < e && s[p] == '@') ++p; }       // read and dropped: stereo travels as wedges
    if (p < e && s[p] == 'H') {
        ++p; *hcount = 1;
        if (p < e && is_digit(s[p])) { *hcount = s[p] - '0'; ++p; }
    }
    if (p < e && (s[p] == '+' || s[p] == '-')) {
        const unsigned char sign = s[p];
        int k = 0, v;
        while (p < e && s[p] == sign) { ++k; ++p; }
        if (k == 1 && p < e && is_digit(s[p])) {
            v = 0;
            while (p < e && is_digit(s[p])) {
                v = v * 10 + (s[p] - '0');
                if (v > 15) return false;
                ++p;
            }
        } else v = k;
        if (v > 15) return false;
        *charge = sign == '+' ? v : -v;
    }
    if (p < e && s[p] == ':') {
        ++p;
        if (p >= e || !is_digit(s[p])) return false;
        while (p < e && is_digit(s[p])) ++p;
    }
    *isotope = iso;
    return p == e;
}

__device__ __forceinline__ bool bytes_are(const unsigned char* s, int n, const char* lit, int ln) {
    if (n != ln) return false;
    for (int k = 0; k < n; ++k)
        if (s[k] != (unsigned char)lit[k]) return false;
    return true;
}

// One atom: the order of tests of chemical.py:886-903 — brackets stripped, R-group table, abbreviation table, and only then
// the whole symbol as a SMILES atom; no parse = pseudo-atom. *sym receives the three bytes of a molfile's symbol column: the
// element capitalised ('R' and a blank for a parsed '*'), "R#" for a numbered R-group, "R" for every other pseudo-atom. *name
// receives the index of the stripped symbol in the name tables, -1 when it is in neither (expand.hip asks which name it was).
__device__ __forceinline__ unsigned interpret_atom(const SymbolTables* __restrict__ st, const unsigned char* s, int n, unsigned* sym,
                                                   int* name) {
    const bool strip = n >= 2 && s[0] == '[' && s[n - 1] == ']';
    const unsigned char* in = strip ? s + 1 : s;
    const int ni = strip ? n - 2 : n;
    const bool chiral = bytes_are(s, n, "[C@]", 4) || bytes_are(s, n, "[C@@]", 5) || bytes_are(s, n, "[C@H]", 5) ||
                        bytes_are(s, n, "[C@@H]", 6);
    unsigned w = chiral ? 8u : 0u;
    const int hit = table_find(st, in, ni);
    *name = hit;
    unsigned char e0 = 'R', e1 = ' ';
    bool lower = false;
    int h = 0, q = 0, iso = 0;
    if (hit < 0 && parse_smiles_atom(s, n, &e0, &e1, &lower, &h, &q, &iso)) {
        w |= CLS_ATOM | (s[0] == '[' ? 4u : 0u) | (unsigned)h << 4 | (unsigned)(q + 15) << 8 | (unsigned)iso << 13 | (lower ? 1u << 31 : 0u);
        *sym = e0 | (unsigned)e1 << 8 | (unsigned)' ' << 16;
        return w;
    }
    unsigned num = 0;           // 'R' followed by digits carries its number (1..999), R-group table only
    if (hit >= 0 && st->kind[hit] == 1 && ni >= 2 && in[0] == 'R') {
        bool digits = true;
        for (int k = 1; k < ni && digits; ++k) {
            digits = is_digit(in[k]);
            if (digits) num = min(num * 10 + (in[k] - '0'), 1000u);
        }
        if (!digits || num > 999) num = 0;
    }
    int al = min(ni, SYM_ALIAS);
    if (ni > SYM_ALIAS)         // never cut a UTF-8 character in two
        while (al > 0 && (in[al] & 0xC0) == 0x80) --al;
    w |= (num ? CLS_RNUM : CLS_PSEUDO) | (unsigned)(15) << 8 | num << 13 | (unsigned)al << 23 | (strip ? 1u << 30 : 0u);
    *sym = 'R' | (unsigned)(num ? '#' : ' ') << 8 | (unsigned)' ' << 16;
    return w;
}

__device__ __forceinline__ unsigned interpret_atom(const SymbolTables* __restrict__ st, const unsigned char* s, int n, unsigned* sym) {
    int name;
    return interpret_atom(st, s, n, sym, &name);
}

// ---- one molecule of the packed tables (PackedTables, table_types.h) ----
// the flag bits that mean the same in both writers' records (molnextr_hip.h)
constexpr unsigned PT_TOO_LARGE = MNX_MOLFILE_TOO_LARGE, PT_BEYOND_TABLES = MNX_MOLFILE_BEYOND_TABLES;
constexpr unsigned PT_PSEUDO_ATOM = MNX_MOLFILE_PSEUDO_ATOM, PT_TRUNCATED = MNX_MOLFILE_TRUNCATED;
static_assert(PT_TOO_LARGE == MNX_SMILES_TOO_LARGE && PT_BEYOND_TABLES == MNX_SMILES_BEYOND_TABLES &&
              PT_PSEUDO_ATOM == MNX_SMILES_PSEUDO_ATOM && PT_TRUNCATED == MNX_SMILES_TRUNCATED, "one meaning, one value");

// Molecule b: its record, its atoms and bonds, and in `flags` PT_TRUNCATED (a copy of MNX_MOL_TRUNCATED), PT_TOO_LARGE (more than
// the 999 atoms or bonds that three digits count) and PT_BEYOND_TABLES (its records end behind a table). With one of the last two
// the molecule is refused and A and B are not read.
struct Molecule {
    mnx_mol m;
    const mnx_atom* A;
    const mnx_bond* B;
    unsigned flags;
};

__device__ __forceinline__ Molecule admit_molecule(const PackedTables& t, int b) {
    const mnx_mol m = t.mols[b];
    unsigned flags = (m.flags & MNX_MOL_TRUNCATED) ? PT_TRUNCATED : 0u;
    if (m.n_atoms > 999u || m.n_bonds > 999u) flags |= PT_TOO_LARGE;
    if ((unsigned long long)m.atom0 + m.n_atoms > t.n_atom_records || (unsigned long long)m.bond0 + m.n_bonds > t.n_bond_records ||
        (unsigned long long)m.text0 + m.smiles_len > t.n_text_bytes)
        flags |= PT_BEYOND_TABLES;
    return {m, t.atoms + m.atom0, t.bonds + m.bond0, flags};
}

// Every atom of an admitted molecule, by NT threads: info[a] its interpretation, sym[a] the bytes of its symbol column, zeros
// for n_atoms <= a < MAX. Returns whether one of this thread's atoms has a symbol that ends behind the text table.
template <int MAX, int NT>
__device__ __forceinline__ int interpret_atoms(const PackedTables& t, const SymbolTables* __restrict__ st, const Molecule& mol,
                                               unsigned* info, unsigned* sym) {
    int bad = 0;
    for (int a = threadIdx.x; a < MAX; a += NT) {
        unsigned w = 0, s3 = 0;
        if (a < (int)mol.m.n_atoms) {
            const unsigned s0 = mol.A[a].sym0, sl = mol.A[a].sym_len;
            if ((unsigned long long)mol.m.text0 + s0 + sl > t.n_text_bytes) bad = 1;
            else w = interpret_atom(st, t.text + mol.m.text0 + s0, (int)sl, &s3);
        }
        info[a] = w;
        sym[a] = s3;
    }
    return bad;
}

}  // namespace mnx
