// molfile_fields.h — the serial parts of mnx_molfile_read (molfile_read.hip): the fields of one line of a V2000 molfile, the bin of
// one coordinate and the spelling of one atom, as __host__ __device__ functions on one line or one atom, so that
// tools/molread_host.cpp runs the very text a lane of the kernel runs under the host compiler's sanitizers (the precedent:
// kekule_search.h with tools/kekule_host.cpp). The rule stands in include/molnextr_hip.h. No arrays that a lane indexes by a
// variable: the bytes an atom is spelled with go to a sink one by one, which counts them, stores them or collects them.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MF_HD __host__ __device__ inline
#else
#define MF_HD inline
#endif

namespace molfields {

// one line: its bytes in front of the '\n' (and of one '\r' in front of that); a byte the line does not have reads as a blank
struct Line {
    const unsigned char* p;
    unsigned len;
};
MF_HD unsigned at(const Line& l, unsigned k) { return k < l.len ? l.p[k] : (unsigned)' '; }
MF_HD bool is_digit(unsigned c) { return c - '0' < 10u; }
MF_HD bool begins(const Line& l, const char* word, unsigned n) {
    if (l.len < n) return false;
    for (unsigned k = 0; k < n; ++k)
        if (l.p[k] != (unsigned char)word[k]) return false;
    return true;
}

// a numeric field "%<width>d" at byte col0: blanks trimmed, empty = 0, else an optional '-' and 1 to 3 digits; false: anything else
MF_HD bool number(const Line& l, unsigned col0, unsigned width, int* value) {
    unsigned a = col0, b = col0 + width;
    while (a < b && at(l, a) == ' ') ++a;
    while (b > a && at(l, b - 1) == ' ') --b;
    *value = 0;
    if (a == b) return true;
    const bool neg = at(l, a) == '-';
    a += neg;
    if (a == b || b - a > 3) return false;
    int v = 0;
    for (; a < b; ++a) {
        if (!is_digit(at(l, a))) return false;
        v = v * 10 + (int)(at(l, a) - '0');
    }
    *value = neg ? -v : v;
    return true;
}

// a coordinate in the 10 bytes at col0, in units of 1e-4: blanks, an optional '-', digits, optionally '.' and digits; nothing else
MF_HD bool coordinate(const Line& l, unsigned col0, long long* units) {
    unsigned a = col0;
    const unsigned b = col0 + 10;
    while (a < b && at(l, a) == ' ') ++a;
    const bool neg = a < b && at(l, a) == '-';
    a += neg;
    if (a == b || !is_digit(at(l, a))) return false;
    long long whole = 0;
    for (; a < b && is_digit(at(l, a)); ++a) whole = whole * 10 + (long long)(at(l, a) - '0');
    long long frac = 0;
    unsigned n_frac = 0;
    if (a < b && at(l, a) == '.') {
        for (++a; a < b && is_digit(at(l, a)); ++a)
            if (n_frac < 4) { frac = frac * 10 + (long long)(at(l, a) - '0'); ++n_frac; }
    }
    if (a != b) return false;
    for (; n_frac < 4; ++n_frac) frac *= 10;
    const long long v = whole * 10000 + frac;
    *units = neg ? -v : v;
    return true;
}

// floor((2 * t * den + s) / (2 * s)) for 0 <= t < 2^48, den < 2^16, 1 <= s < 2^48: the numerator passes 64 bits, so the quotient
// comes from a shift-and-subtract division of 67 bits by 64
MF_HD unsigned long long scaled(unsigned long long t, unsigned long long den, unsigned long long s) {
    const unsigned __int128 num = (unsigned __int128)t * den * 2u + s;
    const unsigned long long d = 2 * s;
    unsigned long long rem = 0, q = 0;
    for (int bit = 66; bit >= 0; --bit) {
        rem = rem << 1 | (unsigned long long)(num >> bit & 1u);
        q <<= 1;                                   // the quotient is below 2^64: t * den / s < 2^64
        if (rem >= d) { rem -= d; q |= 1u; }
    }
    return q;
}

// the bin of a coordinate u at scale s (fit = 0): round-half-up of u * den / s, inside 0..den; *clamped where it was outside
MF_HD unsigned bin_of(long long u, long long s, unsigned den, bool* clamped) {
    if (u < 0) { *clamped = true; return 0; }
    const unsigned long long q = scaled((unsigned long long)u, den, (unsigned long long)s);
    if (q > den) { *clamped = true; return den; }
    return (unsigned)q;
}

// ---- the 118 elements, two bytes each; number 0: none ----
MF_HD unsigned element_number(unsigned c0, unsigned c1) {
    const char* t =
        "H HeLiBeB C N O F NeNaMgAlSiP S ClArK CaScTiV CrMnFeCoNiCuZnGaGeAsSeBrKrRbSrY ZrNbMoTcRuRhPdAgCdInSnSbTeI XeCsBaLaCePrNdPmSmEuGd"
        "TbDyHoErTmYbLuHfTaW ReOsIrPtAuHgTlPbBiPoAtRnFrRaAcThPaU NpPuAmCmBkCfEsFmMdNoLrRfDbSgBhHsMtDsRgCnNhFlMcLvTsOg";
    if (c1 == 0) c1 = ' ';
    for (unsigned k = 0; k < 118; ++k)
        if ((unsigned char)t[2 * k] == c0 && (unsigned char)t[2 * k + 1] == c1) return k + 1;
    return 0;
}

enum : unsigned { NOTE_LABEL = 1u, NOTE_H_DEFAULT = 2u, NOTE_MARKED = 4u };

// what the file says of one atom
struct Atom {
    unsigned sym[3];            // the symbol column, trimmed
    unsigned sym_len;
    int charge;                 // -15..15
    bool has_iso;               // an M ISO entry names the atom
    unsigned iso;               // its value
    unsigned rgp;               // the value of its M RGP entry, 0 without one
    unsigned valence;           // the atom line's valence field, 0..15
    unsigned order_sum;         // bond orders: classes 1, 5, 6 count 1, class 2 counts 2, class 3 counts 3, class 4 counts 0
    bool aromatic;              // has a class-4 bond
    bool wedge;                 // a wedge line begins at it
    Line alias;                 // len 0: none
};

// the smallest target >= s of the default-valence table, minus s; 0 without one
MF_HD unsigned default_h(unsigned el, int charge, unsigned s) {
    // elements by number: B 5, C 6, N 7, O 8, F 9, P 15, S 16, Cl 17, Br 35, I 53
    unsigned t0 = 0, t1 = 0, t2 = 0;
    if (charge == 0) {
        switch (el) {
            case 5: t0 = 3; break;
            case 6: t0 = 4; break;
            case 7: case 15: t0 = 3; t1 = 5; break;
            case 8: t0 = 2; break;
            case 16: t0 = 2; t1 = 4; t2 = 6; break;
            case 9: case 17: case 35: case 53: t0 = 1; break;
            default: break;
        }
    } else if (charge == 1) {
        if (el == 7 || el == 15) t0 = 4;
        else if (el == 8 || el == 16 || el == 6) t0 = 3;
    } else if (charge == -1) {
        if (el == 6) t0 = 3;
        else if (el == 7) t0 = 2;
        else if (el == 8 || el == 16) t0 = 1;
        else if (el == 5) t0 = 4;
    }
    if (t0 >= s && t0) return t0 - s;
    if (t1 >= s && t1) return t1 - s;
    if (t2 >= s && t2) return t2 - s;
    return 0;
}

template <typename Put>
MF_HD void put_number(unsigned v, Put& put) {
    if (v >= 100) put('0' + v / 100 % 10);
    if (v >= 10) put('0' + v / 10 % 10);
    put('0' + v % 10);
}

// One atom's symbol, byte by byte into put(unsigned); returns NOTE_* bits. The rule's six cases in their order.
template <typename Put>
MF_HD unsigned spell(const Atom& a, Put& put) {
    if (a.alias.len) {
        put('[');
        for (unsigned k = 0; k < a.alias.len; ++k) {
            const unsigned c = a.alias.p[k];
            put(c < 0x20 || c == 0x7f ? (unsigned)'?' : c);
        }
        put(']');
        return NOTE_LABEL;
    }
    const unsigned n = a.sym_len, c0 = n > 0 ? a.sym[0] : 0u, c1 = n > 1 ? a.sym[1] : 0u;
    if (n == 2 && c0 == 'R' && c1 == '#' && a.rgp > 0) {
        put('['); put('R'); put_number(a.rgp, put); put(']');
        return NOTE_LABEL;
    }
    unsigned el, e0, e1 = 0, iso = a.has_iso ? a.iso : 0u;
    const bool star = n == 0 || (n == 2 && c0 == 'R' && c1 == '#') ||
                      (n == 1 && (c0 == 'R' || c0 == 'A' || c0 == 'Q' || c0 == 'L' || c0 == 'X' || c0 == '*'));
    if (n == 1 && (c0 == 'D' || c0 == 'T')) {
        el = 1; e0 = 'H';
        if (!a.has_iso) iso = c0 == 'D' ? 2u : 3u;
    } else if (star) {
        el = 0; e0 = '*';
    } else {
        el = n <= 2 ? element_number(c0, c1) : 0u;
        if (!el) {
            put('[');
            put(c0);
            if (n > 1) put(c1);
            if (n > 2) put(a.sym[2]);
            put(']');
            return NOTE_LABEL;
        }
        e0 = c0; e1 = c1;
    }
    // B C N O P S Se As in lower case on a class-4 bond
    const bool lower = a.aromatic && (el == 5 || el == 6 || el == 7 || el == 8 || el == 15 || el == 16 || el == 34 || el == 33);
    const bool organic = star || el == 5 || el == 6 || el == 7 || el == 8 || el == 15 || el == 16 || el == 9 || el == 17 || el == 35 || el == 53;
    unsigned h;
    bool from_table = false;
    if (a.valence != 0 && !a.aromatic) {
        const unsigned v = a.valence == 15 ? 0u : a.valence;
        h = v > a.order_sum ? v - a.order_sum : 0u;
    } else if (a.aromatic) {
        h = 0;
    } else {
        h = default_h(el, a.charge, a.order_sum);
        from_table = true;
    }
    if (h > 9) h = 9;
    const bool marked = el == 6 && !lower && a.charge == 0 && iso == 0 && a.wedge && h <= 1;
    const bool bracket = a.charge != 0 || iso != 0 || a.valence != 0 || !organic || marked;
    if (lower) e0 += 'a' - 'A';
    if (!bracket) {
        put(e0);
        if (e1) put(e1);
        return 0;
    }
    put('[');
    if (iso) put_number(iso, put);
    put(e0);
    if (e1) put(e1);
    if (marked) put('@');
    if (h) { put('H'); if (h > 1) put('0' + h); }
    if (a.charge) {
        put(a.charge > 0 ? '+' : '-');
        const unsigned m = (unsigned)(a.charge > 0 ? a.charge : -a.charge);
        if (m > 1) put_number(m, put);
    }
    put(']');
    return (from_table ? NOTE_H_DEFAULT : 0u) | (marked ? NOTE_MARKED : 0u);
}

// the charge of an atom line's charge code; -99: no code; *ignored for code 4 (a doublet radical)
MF_HD int charge_of_code(int code, bool* ignored) {
    switch (code) {
        case 0: return 0;
        case 1: return 3;
        case 2: return 2;
        case 3: return 1;
        case 4: *ignored = true; return 0;
        case 5: return -1;
        case 6: return -2;
        case 7: return -3;
        default: return -99;
    }
}

// the fields of an atom line behind its coordinates; false: a rule breaks. The symbol goes to a->sym / sym_len, the atom-block
// charge to a->charge, the valence to a->valence.
MF_HD bool atom_fields(const Line& l, Atom* a, bool* ignored) {
    if (l.len < 31) return false;
    unsigned s0 = 31, s1 = 34;
    while (s0 < s1 && at(l, s0) == ' ') ++s0;
    while (s1 > s0 && at(l, s1 - 1) == ' ') --s1;
    a->sym_len = s1 - s0;
    a->sym[0] = at(l, s0); a->sym[1] = at(l, s0 + 1); a->sym[2] = at(l, s0 + 2);
    int mass, code, val;
    if (!number(l, 34, 2, &mass) || !number(l, 36, 3, &code) || !number(l, 48, 3, &val)) return false;
    if (mass) *ignored = true;
    const int q = charge_of_code(code, ignored);
    if (q == -99 || val < 0 || val > 15) return false;
    a->charge = q;
    a->valence = (unsigned)val;
    return true;
}

// a bond line: 0 ok, 1 SYNTAX, 2 QUERY (with nothing else wrong). *pair_ok: a1 and a2 name two different atoms; cls: the class of
// the line as it "begins at" a1 (1..6); *either: STEREO_EITHER
MF_HD int bond_fields(const Line& l, int n_atoms, int* a1, int* a2, unsigned* cls, bool* pair_ok, bool* either) {
    int ty, st;
    const bool f1 = number(l, 0, 3, a1), f2 = number(l, 3, 3, a2), f3 = number(l, 6, 3, &ty), f4 = number(l, 9, 3, &st);
    *pair_ok = f1 && f2 && *a1 >= 1 && *a1 <= n_atoms && *a2 >= 1 && *a2 <= n_atoms && *a1 != *a2;
    *cls = 0;
    if (!*pair_ok || !f3 || !f4) return 1;
    if (ty < 1 || ty > 8) return 1;
    const bool query = ty > 4;
    unsigned c = (unsigned)ty;
    if (st == 0) {
    } else if (st == 1 && ty == 1) c = 5;
    else if (st == 6 && ty == 1) c = 6;
    else if ((st == 4 && ty == 1) || (st == 3 && ty == 2)) *either = true;
    else return 1;
    if (query) return 2;
    *cls = c;
    return 0;
}

MF_HD unsigned flip(unsigned cls) { return cls == 5 ? 6u : cls == 6 ? 5u : cls; }
MF_HD unsigned order_of(unsigned cls) { return cls == 2 ? 2u : cls == 3 ? 3u : cls == 4 ? 0u : 1u; }

}  // namespace molfields
