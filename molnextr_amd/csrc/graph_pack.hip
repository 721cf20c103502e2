// graph_pack.hip — the dense outputs of mnx_predict* as packed atom / bond / text tables (mnx_graph_pack): what
// CharTokenizer.sequence_to_smiles (reference tokenization.py:464-515) and the pair loop of predict_images (model.py:135-143)
// derive on the host, as three launches on the device.
//   count  one workgroup per image: atoms, bonds and SMILES bytes of the image -> mols[b]
//   scan   exclusive scan of the three counts over the images -> atom0 / bond0 / text0 of every image, totals (tables_out.h)
//   fill   one workgroup per image: text, atom records, bond records behind those offsets
// Every position in the tables follows from a prefix scan: no atomics, the output is the same word for word on every run.
// Where a record's fields go — the words of a record, the capped stores — is tables_out.h too.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/molnextr_hip.h"
#include "atom_walk.h"
#include "dec_types.h"       // TokenClasses: the ids are walked with the model's token classes (atom_walk.h)
#include "table_passes.h"
#include "tables_out.h"

namespace mnx {
namespace {

constexpr int GP_THREADS = 256;
constexpr int GP_T = 512;            // ids of a row held in LDS (mnx_confidence's limit)
constexpr int GP_ATOMS = 256;        // atoms a row of GP_T ids can hold (an atom takes at least 3 ids): LDS span tables

// What count and fill both need of one row, held in LDS.
struct RowLds {
    int seq[GP_T];
    unsigned char fl[256];
    unsigned char vlen[256];
    int red[GP_THREADS];
};

// Stages the row's ids, the token classes and the name lengths; returns n = ids of the row and sets *end to the position of the
// first '<eos>' / '<pad>' (n when there is none): the ids in front of it spell the SMILES.
__device__ __forceinline__ int stage_row(RowLds& L, const int* __restrict__ tokens, const int* __restrict__ lens,
                                         const TokenClasses* __restrict__ tc, const VocabText* __restrict__ vt, int row, int T,
                                         int* end) {
    const int tid = threadIdx.x;
    const int n = max(min(min(lens[row], T), GP_T), 0);
    int first = n;
    for (int i = tid; i < n; i += GP_THREADS) {
        const int t = tokens[(size_t)row * T + i];
        L.seq[i] = t;
        if ((t == 2 || t == 0) && i < first) first = i;
    }
    for (int i = tid; i < 256; i += GP_THREADS) { L.fl[i] = tc->flags[i]; L.vlen[i] = vt->len[i]; }
    L.red[tid] = first;
    __syncthreads();
    for (int w = GP_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) L.red[tid] = min(L.red[tid], L.red[tid + w]);
        __syncthreads();
    }
    *end = L.red[0];
    __syncthreads();
    return n;
}

// bytes id t contributes to the SMILES: its name's, nothing for a coordinate bin (or an id outside the vocabulary)
__device__ __forceinline__ unsigned name_bytes(const RowLds& L, int t, int x0) {
    return (unsigned)t < (unsigned)min(x0, 256) ? L.vlen[t] : 0u;
}

__global__ __launch_bounds__(GP_THREADS) void graph_count_kernel(
        const int* __restrict__ tokens, const int* __restrict__ lens, const TokenClasses* __restrict__ tc,
        const VocabText* __restrict__ vt, int T, int kmax, const int* __restrict__ n_atoms,
        const unsigned char* __restrict__ edges, const double* __restrict__ overall, mnx_mol* __restrict__ mols) {
    __shared__ RowLds L;
    __shared__ unsigned scan[2 * GP_THREADS];
    __shared__ int walk_k;
    const int row = blockIdx.x, tid = threadIdx.x;
    int end;
    const int n = stage_row(L, tokens, lens, tc, vt, row, T, &end);
    if (tid == 0) walk_k = atom_walk(L.seq, n, L.fl, tc, [](int, int, int) {});
    const int x0 = tc->x0;
    unsigned bytes = 0;
    for (int i = tid; i < end; i += GP_THREADS) bytes += name_bytes(L, L.seq[i], x0);
    unsigned text_total, bond_total;
    block_scan_excl<GP_THREADS>(bytes, scan, &text_total);         // its barriers also publish walk_k
    const int k = min(walk_k, kmax);
    const int kb = min(k, max(n_atoms[row], 0));                   // rows / columns of `edges` that are defined
    const unsigned char* e = edges + (size_t)row * kmax * kmax;
    unsigned nb = 0;
    for (int i = tid; i < kb; i += GP_THREADS)
        for (int j = i + 1; j < kb; ++j) nb += e[(size_t)i * kmax + j] != 0;
    block_scan_excl<GP_THREADS>(nb, scan, &bond_total);
    if (tid == 0)
        store_mol_counts(&mols[row], (unsigned)k, bond_total, text_total, walk_k > kmax ? 1u : 0u, overall ? overall[row] : 0.0);
}

__global__ __launch_bounds__(GP_THREADS) void graph_fill_kernel(
        const int* __restrict__ tokens, const int* __restrict__ lens, const TokenClasses* __restrict__ tc,
        const VocabText* __restrict__ vt, int T, int kmax, const int* __restrict__ atom_idx,
        const int* __restrict__ n_atoms, const unsigned char* __restrict__ edges, const double* __restrict__ atom_scores,
        const double* __restrict__ edge_scores, const TablesOut o) {
    __shared__ RowLds L;
    __shared__ unsigned scan[2 * GP_THREADS];
    __shared__ unsigned off[GP_T + 1];               // byte offset of every id inside the image's SMILES
    __shared__ unsigned char vname[256 * 8];
    __shared__ short span0[GP_ATOMS], span1[GP_ATOMS];   // atom a: symbol ids [span0, span1), x at span1, y at span1 + 1
    const int row = blockIdx.x, tid = threadIdx.x;
    int end;
    const int n = stage_row(L, tokens, lens, tc, vt, row, T, &end);
    for (int i = tid; i < 256 * 8; i += GP_THREADS) vname[i] = vt->name[i >> 3][i & 7];
    if (tid == 0)
        atom_walk(L.seq, n, L.fl, tc, [&](int a, int i0, int j) {
            if (a < GP_ATOMS) { span0[a] = (short)i0; span1[a] = (short)j; }
        });
    const mnx_mol m = o.mols[row];
    const int x0 = tc->x0, y0 = tc->y0;

    // ---- text: per-id byte offsets by a prefix scan (two neighbouring ids per thread), then every id copies its name ----
    const int i0 = 2 * tid, i1 = 2 * tid + 1;
    const unsigned b0 = i0 < end ? name_bytes(L, L.seq[i0], x0) : 0u, b1 = i1 < end ? name_bytes(L, L.seq[i1], x0) : 0u;
    unsigned total;
    const unsigned ex = block_scan_excl<GP_THREADS>(b0 + b1, scan, &total);     // its barriers publish vname and the spans
    off[i0] = ex;
    off[i1] = ex + b0;
    if (tid == GP_THREADS - 1) off[GP_T] = total;
    __syncthreads();
    for (int i = tid; i < end; i += GP_THREADS) {
        const int t = L.seq[i];
        put_text(o, m.text0 + off[i], vname + (t & 255) * 8, name_bytes(L, t, x0));      // no bytes for an id beyond 255
    }

    // ---- atoms: one record per atom of the walk ----
    const int k = (int)m.n_atoms;
    for (int a = tid; a < k; a += GP_THREADS) {
        const int s0 = span0[a], s1 = span1[a];
        put_atom(o, (unsigned long long)m.atom0 + a, atom_word0(off[s0], off[s1] - off[s0], (unsigned)atom_idx[(size_t)row * kmax + a]),
                 atom_word1((unsigned)(L.seq[s1] - x0), (unsigned)(L.seq[s1 + 1] - y0)),
                 score_word(atom_scores ? atom_scores[(size_t)row * kmax + a] : 0.0));
    }

    // ---- bonds: ordered compaction — row counts, a scan over the rows (tiles of GP_THREADS rows with a carry), then every
    //      row writes its own bonds in column order ----
    const int kb = min(k, max(n_atoms[row], 0));
    const unsigned char* e = edges + (size_t)row * kmax * kmax;
    const double* es = edge_scores ? edge_scores + (size_t)row * kmax * kmax : nullptr;
    unsigned carry = 0;
    for (int base = 0; base < kb; base += GP_THREADS) {
        const int i = base + tid;
        unsigned cnt = 0;
        if (i < kb)
            for (int j = i + 1; j < kb; ++j) cnt += e[(size_t)i * kmax + j] != 0;
        unsigned tile_total;
        unsigned at = carry + block_scan_excl<GP_THREADS>(cnt, scan, &tile_total);
        carry += tile_total;
        if (i < kb && cnt)
            for (int j = i + 1; j < kb; ++j) {
                const unsigned ty = e[(size_t)i * kmax + j];
                if (!ty) continue;
                put_bond(o, (unsigned long long)m.bond0 + at, bond_word0((unsigned)i, (unsigned)j, ty, e[(size_t)j * kmax + i]),
                         score_word(es ? es[(size_t)i * kmax + j] : 0.0));
                ++at;
            }
    }
}

}  // namespace

hipError_t graph_pack_enqueue(const TokenClasses* tc_dev, const VocabText* vt_dev, const int* tokens, const int* lens, int n,
                              int T, int kmax, const int* atom_idx, const int* n_atoms, const unsigned char* edges,
                              const double* atom_scores, const double* edge_scores, const double* overall, const TablesOut& o,
                              unsigned* totals, hipStream_t s) {
    hipLaunchKernelGGL(graph_count_kernel, dim3(n), dim3(GP_THREADS), 0, s, tokens, lens, tc_dev, vt_dev, T, kmax, n_atoms,
                       edges, overall, o.mols);
    hipLaunchKernelGGL(mol_scan_kernel, dim3(1), dim3(MOL_SCAN_THREADS), 0, s, o, n, totals);
    hipLaunchKernelGGL(graph_fill_kernel, dim3(n), dim3(GP_THREADS), 0, s, tokens, lens, tc_dev, vt_dev, T, kmax, atom_idx,
                       n_atoms, edges, atom_scores, edge_scores, o);
    return hipGetLastError();
}

}  // namespace mnx
