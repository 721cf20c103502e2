// molread_host.cpp — the serial parts of mnx_molfile_read (molnextr_amd/csrc/molfile_fields.h: the fields of a line, the bin of a
// coordinate, the spelling of an atom) as a program on the host, so that the host compiler's sanitizers see the very text a lane
// of the kernel runs:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/molread_host.cpp -o molread_host
// Around them stands a plain sequential reader after the rule of include/molnextr_hip.h — one loop where the kernel has lanes, scans
// and LDS atomics. stdin: the number of cases, a newline; per case a line `fit sx sy den n_bytes`, then the file's n_bytes bytes and
// a newline. stdout, per case: a line `flags err_line n_marked n_atoms n_bonds`, per atom `x_bin y_bin symbol-in-hex`, per bond
// `i j type rev` (sorted by i, then j). Exit status 2 and a message on stderr for input that is no such description.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../molnextr_amd/csrc/molfile_fields.h"

namespace mf = molfields;

enum : unsigned { SYNTAX = 1, TOO_LARGE = 2, QUERY = 16, STEREO_EITHER = 32, H_DEFAULT = 64, CLAMPED = 128, IGNORED = 256, LABEL = 512 };

struct StringSink {
    std::string s;
    void operator()(unsigned c) { s.push_back((char)c); }
};

struct Result {
    unsigned flags = 0, err_line = 0, n_marked = 0;
    std::vector<std::string> symbols;
    std::vector<unsigned> xb, yb;
    std::vector<unsigned> bonds;        // i << 10 | j | type << 20 | rev << 23
};

static Result refused(unsigned flag, unsigned line) {
    Result r;
    r.flags = flag;
    r.err_line = line;
    return r;
}

static Result read_file(const std::vector<unsigned char>& data, int fit, long long sx, long long sy, unsigned den) {
    const unsigned L = (unsigned)data.size();
    if (L > 262144u) return refused(TOO_LARGE, 0);
    if (L == 0) return Result();
    const unsigned char* f = data.data();
    std::vector<mf::Line> lines;
    for (unsigned s = 0, p = 0; p <= L; ++p) {
        if (p == L) {
            if (s < L) lines.push_back(mf::Line{f + s, L - s});
        } else if (f[p] == '\n') {
            unsigned e = p;
            if (e > s && f[e - 1] == '\r') --e;
            lines.push_back(mf::Line{f + s, e - s});
            s = p + 1;
        }
    }
    const unsigned n_lines = (unsigned)lines.size(), NONE = 0xffffffffu;
    unsigned e0 = NONE;
    for (unsigned l = 0; l < n_lines && l < 8192u && e0 == NONE; ++l)
        if (mf::begins(lines[l], "M  END", 6)) e0 = l;
    if (e0 == NONE && n_lines > 8192u) return refused(TOO_LARGE, 0);
    unsigned err = NONE;
    auto fail = [&](unsigned line_no, bool query = false) { err = std::min(err, 2u * line_no + (query ? 1u : 0u)); };
    const unsigned n_read = e0 != NONE ? e0 + 1 : n_lines, p_end = e0 != NONE ? e0 : n_lines;
    if (e0 == NONE) fail(n_lines + 1);
    int na = 0, nb = 0;
    if (n_read < 4) {
        fail(n_read + 1);
    } else {
        const mf::Line c = lines[3];
        if (!mf::number(c, 0, 3, &na) || !mf::number(c, 3, 3, &nb) || na < 0 || nb < 0) { fail(4); na = nb = 0; }
        for (unsigned p = 0; p + 5 <= c.len; ++p)
            if (std::string((const char*)c.p + p, 5) == "V3000") fail(4);
    }
    const unsigned p0 = 4u + (unsigned)na + (unsigned)nb;
    if (p0 > n_read) fail(n_read + 1);

    Result r;
    std::vector<unsigned> order_sum((size_t)na, 0u), chg((size_t)na, 0u), iso((size_t)na, 0u), rgp((size_t)na, 0u), alias((size_t)na, 0u);
    std::vector<char> aromatic((size_t)na, 0), wedge((size_t)na, 0);
    std::vector<unsigned> keys;
    for (int m = 0; m < nb; ++m) {
        const unsigned l = 4u + (unsigned)na + (unsigned)m;
        if (l >= n_read) continue;
        int a1, a2;
        unsigned cls;
        bool pair_ok, either = false;
        const int res = mf::bond_fields(lines[l], na, &a1, &a2, &cls, &pair_ok, &either);
        if (res) fail(l + 1, res == 2);
        if (!pair_ok) continue;
        const unsigned i = (unsigned)std::min(a1, a2) - 1u, j = (unsigned)std::max(a1, a2) - 1u;
        for (unsigned k : keys)
            if ((k & 0xfffffu) == (i << 10 | j)) fail(l + 1);
        keys.push_back(i << 10 | j | (a1 < a2 ? cls : mf::flip(cls)) << 20 | (a1 < a2 ? mf::flip(cls) : cls) << 23);
        if (res == 0) {
            order_sum[(size_t)a1 - 1] += mf::order_of(cls);
            order_sum[(size_t)a2 - 1] += mf::order_of(cls);
            if (cls == 4) aromatic[(size_t)a1 - 1] = aromatic[(size_t)a2 - 1] = 1;
            if (cls == 5 || cls == 6) wedge[(size_t)a1 - 1] = 1;
            if (either) r.flags |= STEREO_EITHER;
        }
    }
    bool any_chg = false;
    for (unsigned l = p0; l < p_end; ++l) {
        const mf::Line ln = lines[l];
        if (mf::begins(ln, "A  ", 3)) {
            int atom;
            if (!mf::number(ln, 3, 3, &atom) || atom < 1 || atom > na || l + 1 >= p_end) fail(l + 1);
            else if (lines[l + 1].len > 70) fail(l + 2);
            else alias[(size_t)atom - 1] = l + 2;
            ++l;                                         // the next line is that alias's text
        } else if (mf::begins(ln, "M  CHG", 6) || mf::begins(ln, "M  ISO", 6) || mf::begins(ln, "M  RGP", 6)) {
            const unsigned kind = ln.p[3];
            any_chg |= kind == 'C';
            int cnt;
            if (!mf::number(ln, 6, 3, &cnt) || cnt < 1 || cnt > 8) { fail(l + 1); continue; }
            for (int e = 0; e < cnt; ++e) {
                int atom, v;
                const bool ok = mf::number(ln, 10u + 8u * (unsigned)e, 3, &atom) && mf::number(ln, 14u + 8u * (unsigned)e, 3, &v) && atom >= 1 &&
                                atom <= na && (kind == 'C' ? v >= -15 && v <= 15 : v >= 0);
                if (!ok) { fail(l + 1); break; }
                (kind == 'C' ? chg : kind == 'I' ? iso : rgp)[(size_t)atom - 1] = 1u << 10 | (unsigned)(kind == 'C' ? v + 15 : v);
            }
        } else {
            r.flags |= IGNORED;
        }
    }
    std::vector<long long> ux((size_t)na, 0), uy((size_t)na, 0);
    std::vector<mf::Atom> atoms((size_t)na);
    for (int k = 0; k < na; ++k) {
        const unsigned l = 4u + (unsigned)k;
        if (l >= n_read) continue;
        bool ignored = false;
        if (!mf::atom_fields(lines[l], &atoms[(size_t)k], &ignored) || !mf::coordinate(lines[l], 0, &ux[(size_t)k]) ||
            !mf::coordinate(lines[l], 10, &uy[(size_t)k]))
            fail(l + 1);
        if (ignored) r.flags |= IGNORED;
    }
    if (err != NONE) return refused(err & 1u ? QUERY : SYNTAX, err >> 1);

    long long minx = 0, miny = 0;
    unsigned long long span = 1;
    if (fit && na > 0) {
        minx = *std::min_element(ux.begin(), ux.end());
        miny = *std::min_element(uy.begin(), uy.end());
        span = (unsigned long long)std::max({*std::max_element(ux.begin(), ux.end()) - minx, *std::max_element(uy.begin(), uy.end()) - miny, 1ll});
    }
    for (int k = 0; k < na; ++k) {
        mf::Atom& a = atoms[(size_t)k];
        const size_t z = (size_t)k;
        if (chg[z]) a.charge = (int)(chg[z] & 1023u) - 15;
        else if (any_chg) a.charge = 0;
        a.has_iso = iso[z] != 0; a.iso = iso[z] & 1023u;
        a.rgp = rgp[z] & 1023u;
        a.order_sum = order_sum[z]; a.aromatic = aromatic[z]; a.wedge = wedge[z];
        a.alias = alias[z] ? lines[alias[z] - 1] : mf::Line{f, 0};
        StringSink sink;
        const unsigned got = mf::spell(a, sink);
        bool clamped = false;
        if (fit) {
            r.xb.push_back((unsigned)mf::scaled((unsigned long long)(ux[z] - minx), den, span));
            r.yb.push_back(den - (unsigned)mf::scaled((unsigned long long)(uy[z] - miny), den, span));
        } else {
            r.xb.push_back(mf::bin_of(ux[z], sx, den, &clamped));
            r.yb.push_back(den - mf::bin_of(uy[z], sy, den, &clamped));
        }
        r.flags |= (clamped ? CLAMPED : 0u) | (got & mf::NOTE_LABEL ? LABEL : 0u) | (got & mf::NOTE_H_DEFAULT ? H_DEFAULT : 0u);
        r.n_marked += (got & mf::NOTE_MARKED) != 0;
        r.symbols.push_back(sink.s);
    }
    std::sort(keys.begin(), keys.end(), [](unsigned p, unsigned q) { return (p & 0xfffffu) < (q & 0xfffffu); });
    r.bonds = keys;
    return r;
}

int main() {
    long cases;
    if (std::scanf("%ld", &cases) != 1 || cases < 0 || std::getchar() != '\n') {
        std::fprintf(stderr, "molread_host: no number of cases\n");
        return 2;
    }
    for (long c = 0; c < cases; ++c) {
        int fit;
        long long sx, sy;
        unsigned den;
        unsigned long n_bytes;
        if (std::scanf("%d %lld %lld %u %lu", &fit, &sx, &sy, &den, &n_bytes) != 5 || std::getchar() != '\n' || n_bytes > (1ul << 20) || sx < 1 ||
            sy < 1 || sx > 10000000 || sy > 10000000 || den < 1 || den > 65535) {
            std::fprintf(stderr, "molread_host: no `fit sx sy den n_bytes` (case %ld)\n", c);
            return 2;
        }
        std::vector<unsigned char> data(n_bytes);
        if ((n_bytes && std::fread(data.data(), 1, n_bytes, stdin) != n_bytes) || std::getchar() != '\n') {
            std::fprintf(stderr, "molread_host: the file is shorter than it says (case %ld)\n", c);
            return 2;
        }
        const Result r = read_file(data, fit, sx, sy, den);
        std::printf("%u %u %u %zu %zu\n", r.flags, r.err_line, r.n_marked, r.symbols.size(), r.bonds.size());
        for (size_t k = 0; k < r.symbols.size(); ++k) {
            std::printf("%u %u ", r.xb[k], r.yb[k]);
            for (unsigned char ch : r.symbols[k]) std::printf("%02x", ch);
            std::printf("\n");
        }
        for (unsigned w : r.bonds) std::printf("%u %u %u %u\n", w >> 10 & 1023u, w & 1023u, w >> 20 & 7u, w >> 23 & 7u);
    }
    return 0;
}
