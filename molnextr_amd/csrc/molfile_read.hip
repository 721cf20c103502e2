// molfile_read.hip — V2000 molfiles read into the packed molecule tables (mnx_molfile_read): the inverse of mnx_molfile_pack, so
// that 2D coordinates and wedge flags — what the stereo writers read — enter the chain of passes from a caller's own files.
//   count  one workgroup per file: lines, atoms, bonds, properties, the refusals -> mols[b] (n_atoms, n_bonds, smiles_len), recs[b]
//   scan   exclusive scan of the three counts over the files -> atom0 / bond0 / text0, totals (tables_out.h)
//   fill   one workgroup per file: the same reading again, the records behind those offsets
// The rule stands in include/molnextr_hip.h; the fields of a line and the spelling of an atom are molfile_fields.h. A file of up
// to 262144 bytes stays in global memory; what lies in LDS is where its lines begin (8192 at the most) and a few words per atom:
//   parallel   newlines counted per lane over tiles of 4096 bytes, a workgroup scan with a running carry -> the line starts; the
//              first line that begins "M  END" is a minimum
//   parallel   one lane per bond line: the order sum, the aromatic and the wedge bit of its two atoms (LDS add / or), its key
//              i << 10 | j; then its rank among the keys, where an equal key on an earlier line is the duplicate
//   parallel   the property lines in 256 runs of neighbouring lines: whether a line is an alias's text depends on how many
//              "A  " lines stand directly in front of it, which a run knows from the runs in front (one word each); an entry of
//              M CHG / ISO / RGP and an alias go to their atom by LDS atomicMax on a key with the file order in its high bits
//   parallel   one lane per atom line: its fields, its symbol's length; a workgroup scan of the lengths -> sym0
// Every position comes from a scan or a rank; the lowest error line is a minimum, "the later entry wins" a maximum: no result
// depends on the order of execution. Where a record's fields go is tables_out.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/molnextr_hip.h"
#include "molfile_fields.h"
#include "table_passes.h"
#include "tables_out.h"

namespace mnx {
namespace {

namespace mf = molfields;

constexpr int MR_THREADS = 256;
constexpr int MR_PER = 16;                               // neighbouring bytes per thread and tile
constexpr unsigned MR_TILE = MR_THREADS * MR_PER;
constexpr unsigned MR_BYTES = 262144;                    // the longest file read
constexpr unsigned MR_LINES = 8192;                      // the most lines up to "M  END"
constexpr int MR_ATOMS = 1000;                           // per-atom state: three columns hold 999 at the most
constexpr int MR_SCAN_ATOMS = 1024;                      // four neighbouring atoms per thread in the scan of the symbol lengths
constexpr unsigned NO_LINE = 0xffffffffu, NO_ERR = 0xffffffffu, NO_PAIR = 0xffffffffu;
constexpr unsigned ACC_AROMATIC = 1u << 12, ACC_WEDGE = 1u << 13, ACC_SUM = 0xfffu;     // 999 bonds of order 3 stay below 2^12
constexpr unsigned HAS_CHG = 1u << 31;                   // in sh_flags, beside the MNX_MOLREAD_* notes
constexpr unsigned long long BIAS = 1ull << 62;          // a signed coordinate as an unsigned one, for the LDS minimum / maximum

struct CountSink {
    unsigned n;
    __device__ void operator()(unsigned) { ++n; }
};
struct TextSink {
    const TablesOut& o;
    unsigned long long at;
    unsigned n;
    __device__ void operator()(unsigned c) {
        const unsigned char ch = (unsigned char)c;
        put_text(o, at + n, &ch, 1);
        ++n;
    }
};

template <bool FILL>
__global__ __launch_bounds__(MR_THREADS) void molfile_read_kernel(
        const unsigned char* __restrict__ bytes, unsigned n_bytes, const unsigned* __restrict__ offsets,
        const int* __restrict__ scale, int fit, unsigned den, mnx_molread* __restrict__ recs, const TablesOut o) {
    __shared__ unsigned starts[MR_LINES + 1];            // where line l begins; starts[l + 1] - 1 is its '\n'
    __shared__ unsigned chg[MR_ATOMS], iso[MR_ATOMS], rgp[MR_ATOMS];     // (entry's file order + 1) << 10 | value (CHG: + 15); 0: none
    __shared__ unsigned alias[MR_ATOMS];                 // the alias's text line + 1; 0: none
    __shared__ unsigned acc[MR_ATOMS];                   // order sum | ACC_AROMATIC | ACC_WEDGE
    __shared__ unsigned symoff[MR_SCAN_ATOMS];           // first: a symbol's length; then where it begins in the molecule's text
    __shared__ unsigned ent[MR_ATOMS];                   // a bond line: i << 10 | j | type << 20 | rev << 23, NO_PAIR without a pair
    __shared__ unsigned scan[2 * MR_THREADS];
    __shared__ unsigned long long sh_lo[2], sh_hi[2];    // fit: the least and the greatest x and y, biased
    __shared__ unsigned sh_err, sh_end, sh_flags, sh_marked;

    const int b = blockIdx.x, tid = threadIdx.x;
    const unsigned o0 = offsets[b], o1 = offsets[b + 1];

    auto record = [&](unsigned n_atoms, unsigned n_bonds, unsigned len, unsigned flags, unsigned err_line, unsigned n_marked) {
        if (FILL || tid != 0) return;
        store_mol_counts(&o.mols[b], n_atoms, n_bonds, len, 0u, 0.0);
        recs[b] = mnx_molread{flags, err_line, n_marked, 0u};
    };
    mnx_mol mo;
    if (FILL) {
        mo = o.mols[b];
        if (mo.n_atoms == 0) return;        // refused by count, or no atoms and so no bonds (the same for every thread)
    } else {
        if (o0 > o1 || o1 > n_bytes) { record(0, 0, 0, MNX_MOLREAD_BEYOND, 0, 0); return; }
        if (o1 - o0 > MR_BYTES) { record(0, 0, 0, MNX_MOLREAD_TOO_LARGE, 0, 0); return; }
        if (o1 == o0) { record(0, 0, 0, 0, 0, 0); return; }
    }
    const unsigned L = o1 - o0;
    const unsigned char* __restrict__ f = bytes + o0;

    for (int k = tid; k < MR_ATOMS; k += MR_THREADS) chg[k] = iso[k] = rgp[k] = alias[k] = acc[k] = 0;
    for (int k = tid; k < MR_SCAN_ATOMS; k += MR_THREADS) symoff[k] = 0;
    if (tid == 0) {
        starts[0] = 0;
        sh_err = NO_ERR; sh_end = NO_LINE; sh_flags = 0; sh_marked = 0;
        sh_lo[0] = sh_lo[1] = ~0ull; sh_hi[0] = sh_hi[1] = 0;
    }
    __syncthreads();

    // ---- where the lines begin ----
    unsigned nn = 0;                                     // the newlines in front of the tile; in the end all of them
    for (unsigned base = 0; base < L; base += MR_TILE) {
        const unsigned p0 = base + MR_PER * (unsigned)tid;
        unsigned mask = 0;
#pragma unroll
        for (int q = 0; q < MR_PER; ++q)
            if (p0 + q < L && f[p0 + q] == '\n') mask |= 1u << q;
        unsigned tot;
        unsigned idx = nn + block_scan_excl<MR_THREADS>((unsigned)__popc(mask), scan, &tot);
#pragma unroll
        for (int q = 0; q < MR_PER; ++q)
            if (mask >> q & 1u) {
                ++idx;
                if (idx <= MR_LINES) starts[idx] = p0 + q + 1;
            }
        nn += tot;
    }
    __syncthreads();
    const unsigned n_lines = nn + (f[L - 1] != '\n');    // the last line may lack its '\n'
    const unsigned n_kept = min(n_lines, MR_LINES);      // the lines whose beginning is known
    auto line = [&](unsigned l) {                        // line l < n_kept (0-based)
        const unsigned s = starts[l];
        unsigned e = l < nn ? starts[l + 1] - 1u : L;
        if (l < nn && e > s && f[e - 1] == '\r') --e;
        return mf::Line{f + s, e - s};
    };
    unsigned err = NO_ERR;                               // 2 * line + (1: the QUERY rule), so SYNTAX wins a line
    auto fail = [&](unsigned line_no, bool query = false) { err = min(err, 2u * line_no + (query ? 1u : 0u)); };

    for (unsigned l = tid; l < n_kept; l += MR_THREADS)
        if (mf::begins(line(l), "M  END", 6)) atomicMin(&sh_end, l);
    __syncthreads();
    const unsigned e0 = sh_end;
    if (e0 == NO_LINE && n_lines > MR_LINES) { record(0, 0, 0, MNX_MOLREAD_TOO_LARGE, 0, 0); return; }     // the same for every thread
    const unsigned n_read = e0 != NO_LINE ? e0 + 1u : n_lines;       // the lines that are read at all, <= MR_LINES
    const unsigned p_end = e0 != NO_LINE ? e0 : n_lines;             // the property block ends in front of this line
    if (e0 == NO_LINE) fail(n_lines + 1u);

    // ---- the counts line ----
    int na = 0, nb = 0;
    if (n_read < 4) {
        fail(n_read + 1u);
    } else {
        const mf::Line c = line(3);
        if (!mf::number(c, 0, 3, &na) || !mf::number(c, 3, 3, &nb) || na < 0 || nb < 0) { fail(4); na = nb = 0; }
        for (unsigned p = tid; p + 5 <= c.len; p += MR_THREADS)
            if (c.p[p] == 'V' && c.p[p + 1] == '3' && c.p[p + 2] == '0' && c.p[p + 3] == '0' && c.p[p + 4] == '0') fail(4);
    }
    const unsigned p0 = 4u + (unsigned)na + (unsigned)nb;            // the first property line
    if (p0 > n_read) fail(n_read + 1u);                               // an atom or bond line is missing

    // ---- bond lines ----
    unsigned notes = 0;
    for (int m = tid; m < nb; m += MR_THREADS) {
        const unsigned l = 4u + (unsigned)na + (unsigned)m;
        unsigned key = NO_PAIR;
        if (l < n_read) {
            int a1, a2;
            unsigned cls;
            bool pair_ok, either = false;
            const int res = mf::bond_fields(line(l), na, &a1, &a2, &cls, &pair_ok, &either);
            if (res) fail(l + 1u, res == 2);
            if (pair_ok) {
                const unsigned i = (unsigned)min(a1, a2) - 1u, j = (unsigned)max(a1, a2) - 1u;
                const unsigned ci = a1 < a2 ? cls : mf::flip(cls), cj = a1 < a2 ? mf::flip(cls) : cls;
                key = i << 10 | j | ci << 20 | cj << 23;
                if (res == 0) {
                    const unsigned add = mf::order_of(cls) | (cls == 4 ? ACC_AROMATIC : 0u);
                    atomicAdd(&acc[a2 - 1], add & ACC_SUM);
                    atomicAdd(&acc[a1 - 1], add & ACC_SUM);
                    if (add & ACC_AROMATIC) { atomicOr(&acc[a1 - 1], ACC_AROMATIC); atomicOr(&acc[a2 - 1], ACC_AROMATIC); }
                    if (cls == 5 || cls == 6) atomicOr(&acc[a1 - 1], ACC_WEDGE);
                    if (either) notes |= MNX_MOLREAD_STEREO_EITHER;
                }
            }
        }
        ent[m] = key;
    }

    // ---- property lines: 256 runs of neighbouring lines ----
    const unsigned n_prop = p_end > p0 ? p_end - p0 : 0u;
    const unsigned per = (n_prop + MR_THREADS - 1) / MR_THREADS;      // <= 32
    const unsigned l0 = min(p0 + per * (unsigned)tid, p_end), l1 = min(l0 + per, p_end);
    unsigned a_like = 0, tail = 0;                       // bit c: line l0 + c begins "A  "; the "A  " lines at the run's end
    for (unsigned l = l0; l < l1 && l >= p0; ++l) {
        const bool a = mf::begins(line(l), "A  ", 3);
        a_like |= (a ? 1u : 0u) << (l - l0);
        tail = a ? tail + 1u : 0u;
    }
    scan[tid] = (tail == l1 - l0 ? 2u : 0u) | (tail & 1u);           // bit 1: nothing but "A  " lines (or no line)
    __syncthreads();
    unsigned odd = 0;                                    // an odd number of "A  " lines stands directly in front: this line is a text
    for (int u = tid - 1; u >= 0; --u) {
        odd ^= scan[u] & 1u;
        if (!(scan[u] & 2u)) break;
    }
    __syncthreads();                                     // scan is free again
    for (unsigned l = l0; l < l1 && l >= p0; ++l) {
        const bool a = a_like >> (l - l0) & 1u;
        if (odd) { odd = 0; continue; }                  // an alias's text: its "A  " line has dealt with it
        odd = a ? 1u : 0u;
        const mf::Line ln = line(l);
        int cnt;
        if (a) {
            int atom;
            if (!mf::number(ln, 3, 3, &atom) || atom < 1 || atom > na || l + 1 >= p_end) { fail(l + 1u); continue; }
            if (line(l + 1).len > 70) { fail(l + 2u); continue; }
            atomicMax(&alias[atom - 1], l + 2u);
        } else if (mf::begins(ln, "M  CHG", 6) || mf::begins(ln, "M  ISO", 6) || mf::begins(ln, "M  RGP", 6)) {
            const unsigned kind = ln.p[3];               // 'C', 'I' or 'R'
            if (kind == 'C') notes |= HAS_CHG;
            if (!mf::number(ln, 6, 3, &cnt) || cnt < 1 || cnt > 8) { fail(l + 1u); continue; }
            for (int e = 0; e < cnt; ++e) {
                int atom, v;
                const bool ok = mf::number(ln, 10u + 8u * e, 3, &atom) && mf::number(ln, 14u + 8u * e, 3, &v) && atom >= 1 && atom <= na &&
                                (kind == 'C' ? v >= -15 && v <= 15 : v >= 0);
                if (!ok) { fail(l + 1u); break; }
                const unsigned key = ((l - p0) * 8u + (unsigned)e + 1u) << 10 | (unsigned)(kind == 'C' ? v + 15 : v);
                atomicMax(kind == 'C' ? &chg[atom - 1] : kind == 'I' ? &iso[atom - 1] : &rgp[atom - 1], key);
            }
        } else {
            notes |= MNX_MOLREAD_IGNORED;
        }
    }
    if (notes) atomicOr(&sh_flags, notes);
    notes = 0;
    __syncthreads();                                     // ent, acc, the keys and HAS_CHG are complete

    // ---- a bond's rank among the keys; the same pair on an earlier line ----
    for (int m = tid; m < nb; m += MR_THREADS) {
        const unsigned w = ent[m];
        if (w == NO_PAIR) continue;
        unsigned rank = 0;
        bool twice = false;
        for (int x = 0; x < nb; ++x) {
            const unsigned v = ent[x];
            if (v == NO_PAIR) continue;
            rank += (v & 0xfffffu) < (w & 0xfffffu);
            twice |= (v & 0xfffffu) == (w & 0xfffffu) && x < m;
        }
        if (twice) fail(5u + (unsigned)na + (unsigned)m);
        if (FILL) put_bond(o, (unsigned long long)mo.bond0 + rank, bond_word0(w >> 10 & 1023u, w & 1023u, w >> 20 & 7u, w >> 23 & 7u), 0);
    }

    // ---- atom lines ----
    if (fit) {
        for (int k = tid; k < na; k += MR_THREADS) {
            const unsigned l = 4u + (unsigned)k;
            long long ux, uy;
            if (l < n_read && mf::coordinate(line(l), 0, &ux) && mf::coordinate(line(l), 10, &uy)) {
                atomicMin(&sh_lo[0], (unsigned long long)ux + BIAS); atomicMax(&sh_hi[0], (unsigned long long)ux + BIAS);
                atomicMin(&sh_lo[1], (unsigned long long)uy + BIAS); atomicMax(&sh_hi[1], (unsigned long long)uy + BIAS);
            }
        }
        __syncthreads();
    }
    const bool any_chg = sh_flags & HAS_CHG;
    long long sx = 100000, sy = 100000;
    if (scale) { sx = min(max(scale[2 * b], 1), 10000000); sy = min(max(scale[2 * b + 1], 1), 10000000); }
    unsigned long long span = 1;
    if (fit && na > 0 && sh_lo[0] <= sh_hi[0]) span = max(max(sh_hi[0] - sh_lo[0], sh_hi[1] - sh_lo[1]), 1ull);

    // atom k: its symbol into the sink, its bins; false where its line breaks a rule or is missing
    auto atom_at = [&](int k, auto& sink, unsigned* xb, unsigned* yb) {
        const unsigned l = 4u + (unsigned)k;
        if (l >= n_read) return false;
        const mf::Line ln = line(l);
        mf::Atom a;
        bool ignored = false, clamped = false;
        long long ux, uy;
        if (!mf::atom_fields(ln, &a, &ignored) || !mf::coordinate(ln, 0, &ux) || !mf::coordinate(ln, 10, &uy)) { fail(l + 1u); return false; }
        const unsigned kc = chg[k], ki = iso[k], kr = rgp[k], al = alias[k], ac = acc[k];
        if (kc) a.charge = (int)(kc & 1023u) - 15;
        else if (any_chg) a.charge = 0;
        a.has_iso = ki != 0; a.iso = ki & 1023u;
        a.rgp = kr & 1023u;
        a.order_sum = ac & ACC_SUM; a.aromatic = ac & ACC_AROMATIC; a.wedge = ac & ACC_WEDGE;
        a.alias = mf::Line{f, 0};
        if (al) { a.alias = line(al - 1u); a.alias.len = min(a.alias.len, 70u); }
        const unsigned got = mf::spell(a, sink);
        if (fit) {
            *xb = (unsigned)mf::scaled((unsigned long long)ux + BIAS - sh_lo[0], den, span);
            *yb = den - (unsigned)mf::scaled((unsigned long long)uy + BIAS - sh_lo[1], den, span);
        } else {
            *xb = mf::bin_of(ux, sx, den, &clamped);
            *yb = den - mf::bin_of(uy, sy, den, &clamped);
        }
        notes |= (ignored ? MNX_MOLREAD_IGNORED : 0u) | (clamped ? MNX_MOLREAD_CLAMPED : 0u) | (got & mf::NOTE_LABEL ? MNX_MOLREAD_LABEL : 0u) |
                 (got & mf::NOTE_H_DEFAULT ? MNX_MOLREAD_H_DEFAULT : 0u);
        if (!FILL && (got & mf::NOTE_MARKED)) atomicAdd(&sh_marked, 1u);
        return true;
    };
    for (int k = tid; k < na; k += MR_THREADS) {
        CountSink sink{0};
        unsigned xb, yb;
        if (atom_at(k, sink, &xb, &yb)) symoff[k] = sink.n;
    }
    if (notes) atomicOr(&sh_flags, notes);
    if (err != NO_ERR) atomicMin(&sh_err, err);
    __syncthreads();

    // ---- where each symbol begins: a scan of the lengths, four neighbouring atoms per thread ----
    unsigned len4[4], sum4 = 0, text_len;
#pragma unroll
    for (int q = 0; q < 4; ++q) { len4[q] = symoff[4 * tid + q]; sum4 += len4[q]; }
    unsigned at4 = block_scan_excl<MR_THREADS>(sum4, scan, &text_len);
    if (!FILL) {
        const unsigned e = sh_err;
        if (e != NO_ERR) record(0, 0, 0, e & 1u ? MNX_MOLREAD_QUERY : MNX_MOLREAD_SYNTAX, e >> 1, 0);
        else record((unsigned)na, (unsigned)nb, text_len, sh_flags & ~HAS_CHG, 0, sh_marked);
        return;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) { symoff[4 * tid + q] = at4; at4 += len4[q]; }
    __syncthreads();

    // ---- fill: count admitted the file, mo holds its offsets ----
    for (int k = tid; k < na; k += MR_THREADS) {
        TextSink sink{o, (unsigned long long)mo.text0 + symoff[k], 0};
        unsigned xb = 0, yb = 0;
        atom_at(k, sink, &xb, &yb);
        put_atom(o, (unsigned long long)mo.atom0 + (unsigned)k, atom_word0(symoff[k], sink.n, (unsigned)k), atom_word1(xb, yb), 0);
    }
}

}  // namespace

hipError_t molfile_read_enqueue(const unsigned char* bytes, unsigned n_bytes, const unsigned* offsets, int n, const int* scale,
                                int fit, unsigned den, mnx_molread* recs, const TablesOut& o, unsigned* totals, hipStream_t s) {
    return count_scan_fill(molfile_read_kernel<false>, molfile_read_kernel<true>, n, MR_THREADS, o, totals, s, bytes, n_bytes, offsets,
                           scale, fit, den, recs, o);
}

}  // namespace mnx
