// smiles_read.hip — SMILES text read into the packed molecule tables (mnx_smiles_read): the inverse of mnx_smiles_pack, so that
// every pass over mnx_mol / mnx_atom / mnx_bond (canonical ranks, expansion, molfiles) runs on a caller's own strings.
//   count  one workgroup per string: tokens, atoms, bonds, the refusals -> mols[b] (n_atoms, n_bonds, smiles_len) and recs[b]
//   scan   exclusive scan of the three counts over the strings -> atom0 / bond0 / text0, totals (tables_out.h)
//   fill   one workgroup per string: the same reading again, the records behind those offsets
// The rule stands in include/molnextr_hip.h. A string of up to 4096 bytes lies in LDS, 16 neighbouring bytes per thread:
//   parallel   the nearest bracket in front of every byte (a workgroup max scan) -> inside / outside a bracket atom, the bracket
//              errors; the token every outside byte begins (a look at two bytes on either side); the atoms' numbers and the
//              branch depth in front of every token (two workgroup sum scans) -> '.' inside a branch, ')' without a '('
//   one lane   the walk along the tokens that needs a stack: the atom a new atom or a ring number belongs to (the atom in front
//              of a '(' comes back at its ')'), the 100 ring numbers, the bond symbol that waits for its atom; every bond goes
//              into a list with its place among the bonds of its lower atom (the writer's walk, smiles.hip, is the precedent)
//   parallel   the rows of the bond table: a workgroup scan of the bonds per lower atom, then each bond's rank among its row's
//              entries by their higher atom (as smiles.hip orders its lists), which also finds the same pair twice
// Every position comes from a scan or a rank; the lowest error position is a minimum (LDS atomicMin on a value, no position or
// order depends on it). No symbol tables: a bracket atom's bytes are copied, not interpreted. Where a record's fields go is
// tables_out.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/molnextr_hip.h"
#include "table_passes.h"
#include "tables_out.h"

namespace mnx {
namespace {

constexpr int SR_THREADS = 256;
constexpr int SR_BYTES = 4096;                   // the longest string read (the writers' limit)
constexpr int SR_PER = SR_BYTES / SR_THREADS;    // neighbouring bytes per thread
constexpr int SR_ATOMS = 1024;                   // per-atom state; more than SR_LIMIT atoms are refused in front of it
constexpr unsigned SR_LIMIT = 999;               // atoms / bonds, the writers' limit
// bonds before any is refused: at most 998 between neighbouring atoms, and a ring bond takes two ring tokens of the
// 4096 - atoms bytes left: 998 + (4096 - 999) / 2 < 2560
constexpr int SR_ENTRIES = 2560;
constexpr unsigned NONE = 0xffffu;
constexpr unsigned NO_ERR = 0xffffffffu;

enum : unsigned char { K_NONE = 0, K_ATOM, K_BOND, K_OPEN, K_CLOSE, K_DOT, K_RING, K_BAD };

__device__ __forceinline__ bool is_digit(unsigned c) { return c - '0' < 10u; }
__device__ __forceinline__ bool is_bracket(unsigned c) { return c == '[' || c == ']'; }

// inclusive maximum of one value per thread over the workgroup (Hillis-Steele in LDS, the shape of block_scan_excl); buf holds
// 2 * SR_THREADS words. Ends with a barrier.
__device__ __forceinline__ unsigned block_scan_max(unsigned v, unsigned* buf, unsigned* total) {
    const int tid = threadIdx.x;
    int cur = 0;
    buf[tid] = v;
    __syncthreads();
    for (int d = 1; d < SR_THREADS; d <<= 1) {
        const unsigned x = max(buf[cur * SR_THREADS + tid], tid >= d ? buf[cur * SR_THREADS + tid - d] : 0u);
        buf[(cur ^ 1) * SR_THREADS + tid] = x;
        cur ^= 1;
        __syncthreads();
    }
    const unsigned incl = buf[cur * SR_THREADS + tid];
    *total = buf[cur * SR_THREADS + SR_THREADS - 1];
    __syncthreads();
    return incl;
}

// the class of a bond symbol, 0 for none
__device__ __forceinline__ unsigned symbol_type(unsigned c) {
    return c == '=' ? 2u : c == '#' ? 3u : c == ':' ? 4u : c ? 1u : 0u;       // '-' '/' '\\' are single
}

template <bool FILL>
__global__ __launch_bounds__(SR_THREADS) void smiles_read_kernel(
        const unsigned char* __restrict__ bytes, unsigned n_bytes, const unsigned* __restrict__ offsets,
        mnx_read* __restrict__ recs, const TablesOut o) {
    __shared__ unsigned char s[SR_BYTES + 4];            // the string, zeros behind it
    __shared__ unsigned char kind[SR_BYTES];             // the token a byte begins, K_NONE inside a token
    __shared__ unsigned short aux[SR_BYTES];             // first: at a '[' the position of its ']'; then the walk's stack of atoms
    __shared__ unsigned short apos[SR_ATOMS], alen[SR_ATOMS];       // an atom's span; bit 15 of alen: spelled in lower case
    __shared__ unsigned short rowcnt[SR_ATOMS], rowoff[SR_ATOMS];   // bonds whose lower atom it is; bonds in front of that row
    __shared__ unsigned ent[SR_ENTRIES];                 // a bond: i | j << 10 | type << 20
    __shared__ unsigned short epos[SR_ENTRIES];          // its ring closing token, NONE for a bond between neighbouring atoms
    __shared__ unsigned short eidx[SR_ENTRIES];          // first: its place in its row as the walk met it; then its rank by j
    __shared__ unsigned short bucket[SR_ENTRIES];        // the entries row by row
    __shared__ unsigned short ring_tok[100], ring_atom[100];        // an open ring number: its token + 1, its atom
    __shared__ unsigned char ring_sym[100];
    __shared__ unsigned scan[2 * SR_THREADS];
    __shared__ unsigned sh_err, sh_entries, sh_stereo;

    const int b = blockIdx.x, tid = threadIdx.x;
    const unsigned o0 = offsets[b], o1 = offsets[b + 1];

    auto record = [&](unsigned n_atoms, unsigned n_bonds, unsigned len, unsigned flags, unsigned err_pos, unsigned n_rings) {
        if (FILL || tid != 0) return;
        store_mol_counts(&o.mols[b], n_atoms, n_bonds, len, 0u, 0.0);
        recs[b] = mnx_read{flags, err_pos, n_rings, 0u};
    };
    mnx_mol mo;
    if (FILL) {
        mo = o.mols[b];
        if (mo.smiles_len == 0) return;     // refused by count, or the empty string (the same for every thread)
    } else {
        if (o0 > o1 || o1 > n_bytes) { record(0, 0, 0, MNX_READ_BEYOND, 0, 0); return; }
        if (o1 - o0 > (unsigned)SR_BYTES) { record(0, 0, 0, MNX_READ_TOO_LARGE, 0, 0); return; }
        if (o1 == o0) { record(0, 0, 0, 0, 0, 0); return; }
    }
    const int L = (int)(o1 - o0);

    // ---- the string into LDS ----
    for (int p = tid; p < SR_BYTES + 4; p += SR_THREADS) s[p] = p < L ? bytes[(size_t)o0 + p] : 0;
    for (int k = tid; k < SR_ATOMS; k += SR_THREADS) rowcnt[k] = 0;
    if (tid < 100) ring_tok[tid] = 0;
    if (tid == 0) { sh_err = NO_ERR; sh_entries = 0; sh_stereo = 0; }
    __syncthreads();

    const int p0 = SR_PER * tid;
    unsigned err = NO_ERR;
    auto fail = [&](unsigned at) { err = min(err, at); };

    // ---- the nearest bracket in front of every byte (position + 1, 0: none) ----
    unsigned own = 0;
#pragma unroll
    for (int q = 0; q < SR_PER; ++q)
        if (p0 + q < L && is_bracket(s[p0 + q])) own = (unsigned)(p0 + q + 1);
    unsigned last_bracket;
    const unsigned upto = block_scan_max(own, scan, &last_bracket);
    // exclusive: the maximum over the threads in front of this one
    scan[tid] = upto;
    __syncthreads();
    unsigned pb = tid ? scan[tid - 1] : 0u;
    __syncthreads();
    if (tid == 0 && last_bracket && s[last_bracket - 1] == '[') fail(last_bracket - 1);       // never closed

    // ---- the token every byte begins; atoms and branch depth of the thread's bytes ----
    unsigned char kd[SR_PER];
    unsigned n_at = 0, stereo = 0;
    int dsum = 0;
#pragma unroll
    for (int q = 0; q < SR_PER; ++q) {
        const int p = p0 + q;
        unsigned char k = K_NONE;
        if (p < L) {
            const unsigned c = s[p];
            const bool in = pb && s[pb - 1] == '[';          // between a '[' and the next bracket
            if (c == '[') {
                k = K_ATOM;
                if (in) fail(pb - 1);                        // the '[' in front has no ']'
            } else if (c == ']') {
                if (!in) { k = K_BAD; fail((unsigned)p); }   // stray
                else if (pb == (unsigned)p) fail(pb - 1);    // "[]"
                else aux[pb - 1] = (unsigned short)p;
            } else if (in) {
                stereo |= c == '@';
            } else {
                const unsigned c1 = s[p + 1], c2 = s[p + 2], b1 = p >= 1 ? s[p - 1] : 0u, b2 = p >= 2 ? s[p - 2] : 0u;
                switch (c) {
                    case 'B': case 'C': case 'N': case 'O': case 'P': case 'S': case 'F': case 'I':
                    case 'b': case 'c': case 'n': case 'o': case 'p': case 's': case '*': k = K_ATOM; break;
                    case 'l': k = b1 == 'C' ? K_NONE : K_BAD; break;
                    case 'r': k = b1 == 'B' ? K_NONE : K_BAD; break;
                    case '/': case '\\': stereo = 1; k = K_BOND; break;
                    case '-': case '=': case '#': case ':': k = K_BOND; break;
                    case '(': k = K_OPEN; break;
                    case ')': k = K_CLOSE; break;
                    case '.': k = K_DOT; break;
                    case '%': k = is_digit(c1) && is_digit(c2) ? K_RING : K_BAD; break;      // zeros stand behind the string
                    default:
                        if (is_digit(c)) k = (b1 == '%' && is_digit(c1)) || (b2 == '%' && is_digit(b1)) ? K_NONE : K_RING;
                        else k = K_BAD;
                }
                if (k == K_BAD) fail((unsigned)p);
            }
            if (is_bracket(c)) pb = (unsigned)(p + 1);
        }
        kd[q] = k;
        kind[p] = k;
        n_at += k == K_ATOM;
        dsum += k == K_OPEN ? 1 : k == K_CLOSE ? -1 : 0;
    }
    unsigned n_atoms, depth_end;
    unsigned a_at = block_scan_excl<SR_THREADS>(n_at, scan, &n_atoms);
    int depth = (int)block_scan_excl<SR_THREADS>((unsigned)dsum, scan, &depth_end);     // sums modulo 2^32: signed depths
    if (n_atoms > SR_LIMIT) { record(0, 0, 0, MNX_READ_TOO_LARGE, 0, 0); return; }     // the same for every thread
    unsigned n_dots = 0;
#pragma unroll
    for (int q = 0; q < SR_PER; ++q) {
        const int p = p0 + q;
        const unsigned char k = kd[q];
        if (k == K_ATOM) {
            const unsigned c = s[p];
            unsigned len, lower;
            if (c == '[') {
                len = (unsigned)aux[p] - (unsigned)p + 1u;           // garbage for a '[' without ']': that string is refused
                int z = p + 1;
                while (is_digit(s[z])) ++z;                          // the isotope; zeros stand behind the string
                lower = s[z] - 'a' < 26u;
            } else {
                len = (c == 'C' && s[p + 1] == 'l') || (c == 'B' && s[p + 1] == 'r') ? 2u : 1u;
                lower = c - 'a' < 26u;
            }
            apos[a_at] = (unsigned short)p;
            alen[a_at] = (unsigned short)((len & 0x7fffu) | lower << 15);
            ++a_at;
        } else if (k == K_OPEN) {
            ++depth;
        } else if (k == K_CLOSE) {
            if (depth <= 0) fail((unsigned)p);                       // no '(' is open
            --depth;
        } else if (k == K_DOT) {
            if (depth > 0) fail((unsigned)p);                        // inside a branch
            ++n_dots;
        }
    }
    unsigned dots_total;
    block_scan_excl<SR_THREADS>(n_dots, scan, &dots_total);          // ends with a barrier: apos / alen / kind are complete

    // ---- one lane walks the tokens ----
    if (tid == 0) {
        unsigned cur = NONE, a_next = 0, n_ent = 0, d = 0, first_open = 0;
        unsigned pend = 0, pend_at = 0, dot_at = NONE;
        int fresh = 2;                                   // 2: no atom yet in this component; 1: none yet in this branch
        for (int p = 0; p < L; ++p) {
            const unsigned k = kind[p];
            if (k == K_NONE) continue;
            if (pend && k != K_ATOM && k != K_RING) { fail(pend_at); pend = 0; }           // a bond symbol leads nowhere
            if (dot_at != NONE && k != K_ATOM) fail(dot_at);                               // a '.' in front of no component
            dot_at = NONE;
            if (k == K_ATOM) {
                const unsigned a = a_next++;
                if (cur != NONE) {
                    const unsigned ty = pend ? symbol_type(pend) : (alen[cur] & alen[a] & 0x8000u) ? 4u : 1u;
                    if (n_ent < (unsigned)SR_ENTRIES) {
                        ent[n_ent] = cur | a << 10 | ty << 20;
                        epos[n_ent] = (unsigned short)NONE;
                        eidx[n_ent] = rowcnt[cur]++;
                    }
                    ++n_ent;
                }
                cur = a; pend = 0; fresh = 0;
            } else if (k == K_BOND) {
                if (fresh == 2) fail((unsigned)p);
                pend = s[p]; pend_at = (unsigned)p;
            } else if (k == K_OPEN) {
                if (fresh) fail((unsigned)p);
                if (d == 0) first_open = (unsigned)p;
                aux[d++] = (unsigned short)cur;          // d <= the '(' so far < 4096
                fresh = 1;
            } else if (k == K_CLOSE) {
                if (fresh) fail((unsigned)p);
                if (d > 0) cur = aux[--d];               // a ')' without '(' was found above
                fresh = 0;
            } else if (k == K_DOT) {
                if (fresh) fail((unsigned)p);
                cur = NONE; fresh = 2; dot_at = (unsigned)p;
            } else if (k == K_RING) {
                if (fresh) fail((unsigned)p);
                const unsigned r = s[p] == '%' ? (s[p + 1] - '0') * 10u + (s[p + 2] - '0') : s[p] - '0';
                if (!ring_tok[r]) {
                    ring_tok[r] = (unsigned short)(p + 1); ring_atom[r] = (unsigned short)cur; ring_sym[r] = (unsigned char)pend;
                } else {
                    const unsigned a = ring_atom[r], so = ring_sym[r];
                    ring_tok[r] = 0;
                    if (a == cur || (so && pend && so != pend)) fail((unsigned)p);
                    else if (a != NONE && cur != NONE) {
                        const unsigned sym = so ? so : pend, i = min(a, cur), j = max(a, cur);
                        const unsigned ty = sym ? symbol_type(sym) : (alen[i] & alen[j] & 0x8000u) ? 4u : 1u;
                        if (n_ent < (unsigned)SR_ENTRIES) {
                            ent[n_ent] = i | j << 10 | ty << 20;
                            epos[n_ent] = (unsigned short)p;
                            eidx[n_ent] = rowcnt[i]++;
                        }
                        ++n_ent;
                    }
                }
                pend = 0;
            }
        }
        if (pend) fail(pend_at);
        if (dot_at != NONE) fail(dot_at);
        if (d > 0) fail(first_open);                     // the lowest '(' still open
        for (int r = 0; r < 100; ++r)
            if (ring_tok[r]) fail((unsigned)ring_tok[r] - 1u);
        sh_entries = n_ent;
    }
    if (stereo) sh_stereo = 1;                           // every writer stores the same value
    __syncthreads();
    const unsigned n_all = sh_entries;                   // every bond of the string
    const unsigned n_ent = min(n_all, (unsigned)SR_ENTRIES);     // those in the list: all of them (see SR_ENTRIES)

    // ---- the rows of the bond table ----
    constexpr int APER = SR_ATOMS / SR_THREADS;
    unsigned rsum = 0, rv[APER];
#pragma unroll
    for (int q = 0; q < APER; ++q) { rv[q] = rowcnt[APER * tid + q]; rsum += rv[q]; }
    unsigned rtot;
    unsigned roff = block_scan_excl<SR_THREADS>(rsum, scan, &rtot);
#pragma unroll
    for (int q = 0; q < APER; ++q) { rowoff[APER * tid + q] = (unsigned short)roff; roff += rv[q]; }
    __syncthreads();
    for (unsigned e = tid; e < n_ent; e += SR_THREADS) bucket[rowoff[ent[e] & 1023u] + eidx[e]] = (unsigned short)e;
    __syncthreads();
    for (unsigned e = tid; e < n_ent; e += SR_THREADS) {
        const unsigned w = ent[e], i = w & 1023u, j = w >> 10 & 1023u, at = epos[e];
        const unsigned r0 = rowoff[i], r1 = r0 + rowcnt[i];
        unsigned rank = 0;
        for (unsigned x = r0; x < r1; ++x) {
            const unsigned f = bucket[x];
            if (f == e) continue;
            const unsigned jf = ent[f] >> 10 & 1023u;
            rank += jf < j;
            // the pair has a bond already: the later ring closure breaks the rule
            if (jf == j && at != NONE && (epos[f] == NONE || epos[f] < at)) fail(at);
        }
        eidx[e] = (unsigned short)rank;                  // nobody reads another entry's eidx any more
    }
    if (err != NO_ERR) atomicMin(&sh_err, err);
    __syncthreads();
    if (!FILL) {
        const unsigned e = sh_err;
        if (e != NO_ERR) record(0, 0, 0, MNX_READ_SYNTAX, e, 0);
        else if (n_all > SR_LIMIT) record(0, 0, 0, MNX_READ_TOO_LARGE, 0, 0);
        else record(n_atoms, n_ent, (unsigned)L, sh_stereo ? MNX_READ_STEREO_DROPPED : 0u, 0, n_ent + 1u + dots_total - n_atoms);
        return;
    }

    // ---- fill: count admitted the string, mo holds its offsets ----
    for (unsigned k = tid; k < n_atoms; k += SR_THREADS)          // no bins, no scores
        put_atom(o, (unsigned long long)mo.atom0 + k, atom_word0(apos[k], alen[k] & 0x7fffu, k), 0, 0);
    for (unsigned e = tid; e < n_ent; e += SR_THREADS) {
        const unsigned w = ent[e], i = w & 1023u, j = w >> 10 & 1023u, ty = w >> 20;
        put_bond(o, (unsigned long long)mo.bond0 + rowoff[i] + eidx[e], bond_word0(i, j, ty, ty), 0);
    }
    for (int p = tid; p < L; p += SR_THREADS) put_text(o, (unsigned long long)mo.text0 + (unsigned)p, &s[p], 1);
}

}  // namespace

hipError_t smiles_read_enqueue(const unsigned char* bytes, unsigned n_bytes, const unsigned* offsets, int n, mnx_read* recs,
                               const TablesOut& o, unsigned* totals, hipStream_t s) {
    return count_scan_fill(smiles_read_kernel<false>, smiles_read_kernel<true>, n, SR_THREADS, o, totals, s, bytes, n_bytes, offsets, recs, o);
}

}  // namespace mnx
