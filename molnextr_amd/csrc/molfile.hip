// molfile.hip — CTfile V2000 molfiles from the packed molecule tables of mnx_graph_pack (mnx_molfile_pack): the molecule
// that _convert_graph_to_smiles (reference chemical.py:880-926) builds with RDKit — atoms by symbol class, bonds with their
// wedges, the begin atom of a wedge moved to the chiral centre (chemical.py:262-273) — written as text on the device.
//   count  one workgroup per molecule: symbol classes and the molfile's length -> files[b].len / flags
//          (which molecules are admitted and how an atom is read: atom_symbol.h, shared with smiles.hip)
//   scan   exclusive scan of the lengths over the molecules -> files[b].text0, totals
//   fill   one workgroup per molecule: the bytes behind text0
// Every line of a V2000 block has a fixed width (69-byte atom lines, 12-byte bond lines, property lines of 8 entries), so
// every byte position follows from prefix scans: no atomics, the output is the same byte for byte on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/molnextr_hip.h"
#include "atom_symbol.h"
#include "block_scan.h"
#include "table_passes.h"

namespace mnx {

static_assert(sizeof(mnx_molfile) == 16, "record layout of molnextr_hip.h");

namespace {

constexpr int MF_THREADS = 256;
constexpr int MF_MAX = 1024;             // atoms / bonds held in LDS: a molfile counts three digits (999)
constexpr int MF_PER = MF_MAX / MF_THREADS;

constexpr unsigned HEADER_BYTES = 25, COUNTS_BYTES = 40, ATOM_BYTES = 70, BOND_BYTES = 13, END_BYTES = 7;
constexpr unsigned PROP_HEAD = 9, PROP_ENTRY = 8, PROP_PER_LINE = 8, PROP_LINE = PROP_HEAD + PROP_PER_LINE * PROP_ENTRY + 1;

// k-th byte of "%3d" of v, -99 <= v <= 999
__device__ __forceinline__ char d3(int v, int k) {
    const int a = v < 0 ? -v : v;
    if (k == 2) return (char)('0' + a % 10);
    if (k == 1) return a >= 10 ? (char)('0' + a / 10 % 10) : (v < 0 ? '-' : ' ');
    return a >= 100 ? (char)('0' + a / 100) : (v < 0 && a >= 10 ? '-' : ' ');
}

__device__ __forceinline__ unsigned prop_bytes(unsigned k) {     // a property section of k entries: lines of up to 8
    return (k + PROP_PER_LINE - 1) / PROP_PER_LINE * (PROP_HEAD + 1) + k * PROP_ENTRY;
}

// header block and counts line; the six leading bytes of the counts line are the atom and bond counts
__device__ const char MF_HEAD[] = "\n  MolNexTR          2D\n\n" "aaabbb  0  0  0  0  0  0  0  0999 V2000\n";
static_assert(sizeof(MF_HEAD) == HEADER_BYTES + COUNTS_BYTES + 1, "header and counts line");

template <bool FILL>
__global__ __launch_bounds__(MF_THREADS) void molfile_kernel(
        const PackedTables t, const SymbolTables* __restrict__ st, const int* __restrict__ scale, int den,
        mnx_molfile* __restrict__ files, char* __restrict__ out, unsigned out_cap) {
    __shared__ unsigned info[MF_MAX], sym[MF_MAX];
    __shared__ unsigned aoff[MF_MAX], coff[MF_MAX];     // per atom: bytes of the alias lines / packed entry counts in front of it
    __shared__ unsigned bnd[FILL ? MF_MAX : 1];         // fill: i | j << 10 | order << 20 | aromatic << 22, for the valence sums
    __shared__ unsigned scan[2 * MF_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const Molecule mol = admit_molecule(t, b);
    const mnx_mol& m = mol.m;
    const unsigned truncated = mol.flags & PT_TRUNCATED;
    auto record = [&](unsigned len, unsigned flags) {   // count's result; len 0 = refused
        if (tid == 0) { files[b].len = len; files[b].flags = flags; files[b].reserved = 0; }
    };
    unsigned text0 = 0;
    if (FILL) {
        const mnx_molfile f = files[b];
        if (f.len == 0) return;                         // refused by count (the same for every thread)
        text0 = f.text0;
    } else if (mol.flags & (PT_TOO_LARGE | PT_BEYOND_TABLES)) {
        record(0, mol.flags);
        return;
    }
    const int na = (int)m.n_atoms, nb = (int)m.n_bonds;
    const mnx_atom* A = mol.A;
    const mnx_bond* B = mol.B;
    const unsigned char* text = t.text;

    // ---- every atom's interpretation; a record that points beyond its table refuses the molecule ----
    int bad = interpret_atoms<MF_MAX, MF_THREADS>(t, st, mol, info, sym);
    for (int k = tid; k < nb; k += MF_THREADS) {
        const unsigned i = B[k].i, j = B[k].j, ty = B[k].type;
        if (i >= (unsigned)na || j >= (unsigned)na) bad = 1;        // i == j is written as it stands; the SMILES writer refuses it
        if (FILL) bnd[k] = (i & 1023u) | (j & 1023u) << 10 | (ty <= 3 ? ty : (ty == 5 || ty == 6) ? 1u : 0u) << 20 | (ty == 4 ? 1u : 0u) << 22;
    }
    if (!FILL) {
        if (__syncthreads_or(bad)) {
            record(0, truncated | PT_BEYOND_TABLES);
            return;
        }
    } else {
        __syncthreads();
    }

    // ---- positions: MF_PER neighbouring atoms per thread, two scans (alias bytes; CHG | ISO | RGP entries, 10 bits each) ----
    unsigned va[MF_PER], vc[MF_PER], sa = 0, sc = 0;
    int pseudo = 0;
#pragma unroll
    for (int q = 0; q < MF_PER; ++q) {
        const unsigned w = info[MF_PER * tid + q];
        const bool is_atom = MF_PER * tid + q < na;
        const unsigned cls = info_cls(w), al = info_alias(w);
        va[q] = al ? al + 8u : 0u;                       // "A  nnn\n" + the text + "\n"
        vc[q] = !is_atom ? 0u
                         : (info_charge(w) != 0 ? 1u : 0u) | (cls == CLS_ATOM && info_num(w) ? 1u << 10 : 0u) |
                               (cls == CLS_RNUM ? 1u << 20 : 0u);
        pseudo |= is_atom && cls != CLS_ATOM;
        sa += va[q];
        sc += vc[q];
    }
    unsigned alias_total, cnt_total;
    unsigned ea = block_scan_excl<MF_THREADS>(sa, scan, &alias_total);
    unsigned ec = block_scan_excl<MF_THREADS>(sc, scan, &cnt_total);
    const unsigned n_chg = cnt_total & 1023u, n_iso = cnt_total >> 10 & 1023u, n_rgp = cnt_total >> 20 & 1023u;
    const unsigned off_atoms = HEADER_BYTES + COUNTS_BYTES, off_bonds = off_atoms + ATOM_BYTES * na;
    const unsigned off_alias = off_bonds + BOND_BYTES * nb, off_chg = off_alias + alias_total;
    const unsigned off_iso = off_chg + prop_bytes(n_chg), off_rgp = off_iso + prop_bytes(n_iso);
    const unsigned off_end = off_rgp + prop_bytes(n_rgp);
    if (!FILL) {
        pseudo = __syncthreads_or(pseudo);
        record(off_end + END_BYTES, truncated | (pseudo ? PT_PSEUDO_ATOM : 0u));
        return;
    }
#pragma unroll
    for (int q = 0; q < MF_PER; ++q) {
        aoff[MF_PER * tid + q] = ea;
        coff[MF_PER * tid + q] = ec;
        ea += va[q];
        ec += vc[q];
    }
    __syncthreads();

    auto put = [&](unsigned off, char c) {               // nothing is written beyond out_cap
        const unsigned long long at = (unsigned long long)text0 + off;
        if (at < out_cap) out[at] = c;
    };

    // ---- header and counts line ----
    if (tid < (int)(HEADER_BYTES + COUNTS_BYTES)) {
        char c = MF_HEAD[tid];
        const int k = tid - (int)HEADER_BYTES;
        if (k >= 0 && k < 3) c = d3(na, k);
        else if (k >= 3 && k < 6) c = d3(nb, k - 3);
        put(tid, c);
    }

    // ---- atom lines: coordinates in exact integer arithmetic, units of 1e-4 ----
    long long sx = 100000, sy = 100000;
    if (scale) {
        sx = min(max(scale[2 * b], 1), 10000000);
        sy = min(max(scale[2 * b + 1], 1), 10000000);
    }
    for (int a = tid; a < na; a += MF_THREADS) {
        const unsigned w = info[a], s3 = sym[a], o = off_atoms + ATOM_BYTES * a;
        const long long xb = min((int)A[a].x_bin, den), yb = min((int)A[a].y_bin, den);
        const unsigned u[3] = {(unsigned)((2 * xb * sx + den) / (2 * den)), (unsigned)((2 * (den - yb) * sy + den) / (2 * den)), 0u};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned ip = u[c] / 10000u, fp = u[c] % 10000u, oc = o + 10 * c;
            put(oc, ' ');
            put(oc + 1, ip >= 1000 ? (char)('0' + ip / 1000) : ' ');
            put(oc + 2, ip >= 100 ? (char)('0' + ip / 100 % 10) : ' ');
            put(oc + 3, ip >= 10 ? (char)('0' + ip / 10 % 10) : ' ');
            put(oc + 4, (char)('0' + ip % 10));
            put(oc + 5, '.');
            put(oc + 6, (char)('0' + fp / 1000));
            put(oc + 7, (char)('0' + fp / 100 % 10));
            put(oc + 8, (char)('0' + fp / 10 % 10));
            put(oc + 9, (char)('0' + fp % 10));
        }
        put(o + 30, ' ');
        put(o + 31, (char)(s3 & 255u));
        put(o + 32, (char)(s3 >> 8 & 255u));
        put(o + 33, (char)(s3 >> 16 & 255u));
        int val = 0;            // the valence field: bracket atoms of the grammar without an aromatic bond
        if (info_cls(w) == CLS_ATOM && (w & 4u)) {
            int sum = info_h(w);
            bool arom = false;
            for (int k = 0; k < nb; ++k) {
                const unsigned e = bnd[k];
                if ((e & 1023u) == (unsigned)a || (e >> 10 & 1023u) == (unsigned)a) { sum += (int)(e >> 20 & 3u); arom |= (e >> 22 & 1u) != 0; }
            }
            val = arom ? 0 : sum == 0 ? 15 : sum > 14 ? 0 : sum;
        }
        for (int p = 0; p < 35; ++p) {                   // " 0" and eleven "  0" fields, the sixth of them the valence
            char c = p < 2 ? (p == 1 ? '0' : ' ') : ((p - 2) % 3 == 2 ? '0' : ' ');
            if (p >= 14 && p < 17) c = d3(val, p - 14);
            put(o + 34 + p, c);
        }
        put(o + 69, '\n');
    }

    // ---- bond lines: a wedge begins at a chiral carbon of the higher index when the reverse direction is a wedge ----
    for (int k = tid; k < nb; k += MF_THREADS) {
        const unsigned i = B[k].i, j = B[k].j, ty = B[k].type, rv = B[k].rev, o = off_bonds + BOND_BYTES * k;
        const bool swap = (info[j & (MF_MAX - 1)] & 8u) && (rv == 5 || rv == 6);      // j < n_atoms: count checked it
        const unsigned cls = swap ? rv : ty;
        const int a1 = (int)(swap ? j : i) + 1, a2 = (int)(swap ? i : j) + 1;
        const int bt = cls >= 1 && cls <= 4 ? (int)cls : (cls == 5 || cls == 6) ? 1 : 8, stereo = cls == 5 ? 1 : cls == 6 ? 6 : 0;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            put(o + p, d3(a1, p));
            put(o + 3 + p, d3(a2, p));
            put(o + 6 + p, d3(bt, p));
            put(o + 9 + p, d3(stereo, p));
        }
        put(o + 12, '\n');
    }

    // ---- property lines: aliases, then M  CHG, M  ISO, M  RGP in lines of up to eight entries ----
    for (int a = tid; a < na; a += MF_THREADS) {
        const unsigned w = info[a], al = info_alias(w);
        if (al) {
            const unsigned o = off_alias + aoff[a];
            const unsigned char* in = text + m.text0 + A[a].sym0 + (w >> 30 & 1u);
            put(o, 'A'); put(o + 1, ' '); put(o + 2, ' ');
            for (int p = 0; p < 3; ++p) put(o + 3 + p, d3(a + 1, p));
            put(o + 6, '\n');
            for (unsigned k = 0; k < al; ++k) put(o + 7 + k, in[k] < 0x20 || in[k] == 0x7f ? '?' : (char)in[k]);
            put(o + 7 + al, '\n');
        }
        const unsigned cls = info_cls(w);
        const bool has[3] = {info_charge(w) != 0, cls == CLS_ATOM && info_num(w) != 0, cls == CLS_RNUM};
        const int value[3] = {info_charge(w), (int)info_num(w), (int)info_num(w)};
        const unsigned base[3] = {off_chg, off_iso, off_rgp}, total[3] = {n_chg, n_iso, n_rgp};
        const char* tag = "CHGISORGP";
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (!has[q]) continue;
            const unsigned e = coff[a] >> (10 * q) & 1023u, line = e / PROP_PER_LINE, pos = e % PROP_PER_LINE;
            const unsigned o = base[q] + line * PROP_LINE;
            if (pos == 0) {
                const unsigned cnt = min(PROP_PER_LINE, total[q] - line * PROP_PER_LINE);
                put(o, 'M'); put(o + 1, ' '); put(o + 2, ' ');
                for (int p = 0; p < 3; ++p) { put(o + 3 + p, tag[3 * q + p]); put(o + 6 + p, d3((int)cnt, p)); }
                put(o + PROP_HEAD + cnt * PROP_ENTRY, '\n');
            }
            const unsigned oe = o + PROP_HEAD + pos * PROP_ENTRY;
            put(oe, ' ');
            put(oe + 4, ' ');
            for (int p = 0; p < 3; ++p) { put(oe + 1 + p, d3(a + 1, p)); put(oe + 5 + p, d3(value[q], p)); }
        }
    }
    if (tid < (int)END_BYTES) put(off_end + tid, "M  END\n"[tid]);
}

}  // namespace

hipError_t molfile_pack_enqueue(const SymbolTables* st_dev, const PackedTables& t, const int* scale, int coord_bins,
                                mnx_molfile* files, char* out, unsigned out_cap, unsigned* totals, hipStream_t s) {
    const int den = coord_bins - 1;
    hipLaunchKernelGGL(molfile_kernel<false>, dim3(t.n), dim3(MF_THREADS), 0, s, t, st_dev, scale, den, files, out, out_cap);
    hipLaunchKernelGGL(text_scan_kernel<mnx_molfile>, dim3(1), dim3(TEXT_SCAN_THREADS), 0, s, files, t.n, out_cap, totals);
    hipLaunchKernelGGL(molfile_kernel<true>, dim3(t.n), dim3(MF_THREADS), 0, s, t, st_dev, scale, den, files, out, out_cap);
    return hipGetLastError();
}

}  // namespace mnx
