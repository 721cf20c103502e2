// fingerprint.hip — a path fingerprint of every packed molecule (mnx_fingerprint_pack) and the Tanimoto similarity of rows of such
// fingerprints (mnx_tanimoto): the one graded answer behind the chain of passes, where every other comparison is a yes or a no.
// The rule stands in include/molnextr_hip.h ("Path fingerprints"): this library's own, after the idea of Daylight's and RDKit's
// path fingerprints, NOT their bits. One launch each: the outputs have a fixed size, so there is nothing to count and scan.
//   fingerprint  one workgroup per molecule: admission and the atoms' interpretation (atom_symbol.h), then the unsorted neighbour
//                lists and the duplicate test of mol_graph.h. An atom's key is a hash of the bytes the canonical ranks key
//                on (atom_write.h). The work items are the atoms (the paths of no bonds) and
//                the directed bonds, strided over the threads; a thread walks the paths that begin with its bond depth first
//                (path_search.h) on a stack of its own in LDS and sets their bits in one bitset in LDS.
//   tanimoto     a wave per pair of rows, a lane per word: two popcounts, two wave sums, one division.
// LDS atomics count degrees, hand out slots of unsorted lists (a set of paths does not depend on the order of a list), OR bits
// and take one maximum: none of them decides a result, so the words are the same from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/molnextr_hip.h"
#include "atom_symbol.h"
#include "atom_write.h"
#include "mol_graph.h"
#include "table_passes.h"

namespace mnx {

static_assert(sizeof(mnx_fp) == 16, "record layout of molnextr_hip.h");
static_assert(MNX_FP_TOO_LARGE == PT_TOO_LARGE && MNX_FP_BEYOND_TABLES == PT_BEYOND_TABLES && MNX_FP_PSEUDO_ATOM == PT_PSEUDO_ATOM &&
              MNX_FP_TRUNCATED == PT_TRUNCATED && MNX_FP_BAD_BOND == MNX_SMILES_DUPLICATE_BOND, "one meaning, one value");
static_assert(MNX_FP_WORDS == 64 && MNX_FP_MAX_BONDS == paths::MAX_BONDS, "64 words, a lane of a wave each; 8 levels of stack");

namespace {

constexpr int FP_THREADS = MG_THREADS, FP_MAX = MG_MAX, FP_SLOTS = MG_SLOTS;     // the sizes of mol_graph.h

__global__ __launch_bounds__(FP_THREADS) void fingerprint_kernel(
        const PackedTables t, const SymbolTables* __restrict__ st, mnx_fp* __restrict__ recs, unsigned* __restrict__ bits,
        unsigned max_bonds, unsigned max_steps) {
    __shared__ unsigned info[FP_MAX], elem[FP_MAX];       // the atoms' interpretation; then key = info: every atom's key
    __shared__ unsigned off[FP_MAX + 1], cnt[FP_MAX];
    __shared__ unsigned lst[FP_SLOTS];                    // the lists as the bonds came: paths::entry
    __shared__ unsigned scan[2 * FP_THREADS];
    __shared__ unsigned stk[paths::LEVELS * FP_THREADS];  // level l of thread tid: stk[l * FP_THREADS + tid], a bank per lane
    __shared__ unsigned set[MNX_FP_WORDS];
    __shared__ unsigned most;                             // the largest number of paths from one directed bond
    const int b = blockIdx.x, tid = threadIdx.x;
    const Molecule mol = admit_molecule(t, b);
    const mnx_mol& m = mol.m;
    unsigned* out = bits + (size_t)b * MNX_FP_WORDS;
    auto refuse = [&](unsigned flags) {                   // no fingerprint: 64 zero words
        if (tid < MNX_FP_WORDS) out[tid] = 0u;
        if (tid == 0) recs[b] = mnx_fp{flags, 0u, flags & MNX_FP_LIMIT ? 0xFFFFFFFFu : 0u, 0u};
    };
    if (mol.flags & (PT_TOO_LARGE | PT_BEYOND_TABLES)) { refuse(mol.flags); return; }
    const unsigned base_flags = mol.flags & PT_TRUNCATED;
    const int na = (int)m.n_atoms, nb = (int)m.n_bonds;
    const mnx_bond* B = mol.B;

    // ---- every atom's interpretation; a symbol that ends behind the text table refuses the molecule ----
    int bad = interpret_atoms<FP_MAX, FP_THREADS>(t, st, mol, info, elem), pseudo = 0;
    for (int a = tid; a < FP_MAX; a += FP_THREADS) {      // info[a] is this thread's own entry: no barrier in between
        pseudo |= a < na && info_cls(info[a]) != CLS_ATOM;
        cnt[a] = 0;
    }
    if (tid < MNX_FP_WORDS) set[tid] = 0u;
    if (tid == 0) most = 0u;
    if (__syncthreads_or(bad)) { refuse(base_flags | PT_BEYOND_TABLES); return; }
    const unsigned atom_flags = base_flags | (__syncthreads_or(pseudo) ? PT_PSEUDO_ATOM : 0u);

    // ---- the neighbour lists (mol_graph.h); a bad record refuses the molecule, as a duplicate pair does ----
    if (__syncthreads_or(graph_degrees(mol, cnt))) { refuse(atom_flags | MNX_FP_BAD_BOND); return; }
    graph_lists(mol, cnt, off, scan, lst, [&](int k) { return bond_class(B[k].type) + 1u; });      // the bond word; `rev` is not read
    if (__syncthreads_or(graph_duplicate(mol, off, lst))) { refuse(atom_flags | MNX_FP_BAD_BOND); return; }

    // ---- the atom keys: the written bytes of the canonical ranks' initial key, hashed; a thread rewrites its own entries ----
    unsigned* key = info;
    for (int a = tid; a < na; a += FP_THREADS) {
        unsigned h = paths::FNV_BASIS;
        put_atom(info[a], elem[a], 0u, [&](char c) { h = paths::fnv(h, (unsigned)(unsigned char)c); });
        key[a] = paths::fmix32(h);
    }
    __syncthreads();

    // ---- the paths: of no bonds from every atom, of 1 .. max_bonds bonds from every directed bond ----
    auto hit = [&](unsigned p) {
        const unsigned t0 = p & 2047u, t1 = p >> 11 & 2047u;
        atomicOr(&set[t0 >> 5], 1u << (t0 & 31u));        // an OR does not depend on the order of its operands
        atomicOr(&set[t1 >> 5], 1u << (t1 & 31u));
    };
    for (int a = tid; a < na; a += FP_THREADS) hit(paths::atom_hash(key[a]));
    unsigned mine = 0;
    for (int s = tid; s < 2 * nb && mine <= max_steps; s += FP_THREADS)     // beyond the limit a lane stops counting
        mine = max(mine, paths::walk((unsigned)s, off, lst, key, stk + tid, (unsigned)FP_THREADS, max_bonds, max_steps, hit));
    if (mine) atomicMax(&most, mine);                     // nor does a maximum
    __syncthreads();
    if (most > max_steps) { refuse(atom_flags | MNX_FP_LIMIT); return; }

    // ---- the 64 words and the record, written whole ----
    unsigned word = 0, n_bits = 0;
    if (tid < MNX_FP_WORDS) {
        word = set[tid];
        out[tid] = word;
        n_bits = (unsigned)__popc(word);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n_bits += __shfl_xor(n_bits, o, 64);
    }
    if (tid == 0) recs[b] = mnx_fp{atom_flags, n_bits, most, 0u};
}

// pair r: lane l holds word l of both rows
__global__ __launch_bounds__(FP_THREADS) void tanimoto_kernel(const unsigned* __restrict__ a, const unsigned* __restrict__ b, int n,
                                                              unsigned* __restrict__ both, unsigned* __restrict__ either,
                                                              double* __restrict__ similarity) {
    static_assert(MNX_FP_WORDS == 64, "a wave of 64 per pair");
    const int lane = threadIdx.x & 63, r = blockIdx.x * (FP_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= n) return;                                   // a whole wave leaves
    const unsigned x = a[(size_t)r * MNX_FP_WORDS + lane], y = b[(size_t)r * MNX_FP_WORDS + lane];
    unsigned n_and = (unsigned)__popc(x & y), n_or = (unsigned)__popc(x | y);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_and += __shfl_xor(n_and, o, 64);
        n_or += __shfl_xor(n_or, o, 64);
    }
    if (lane != 0) return;
    if (both) both[r] = n_and;
    if (either) either[r] = n_or;
    if (similarity) similarity[r] = n_or ? (double)n_and / (double)n_or : 0.0;     // one correctly rounded division
}

}  // namespace

hipError_t fingerprint_pack_enqueue(const SymbolTables* st_dev, const PackedTables& t, mnx_fp* recs, unsigned* bits,
                                    unsigned max_bonds, unsigned max_steps, hipStream_t s) {
    hipLaunchKernelGGL(fingerprint_kernel, dim3(t.n), dim3(FP_THREADS), 0, s, t, st_dev, recs, bits, max_bonds, max_steps);
    return hipGetLastError();
}

hipError_t tanimoto_enqueue(const unsigned* a, const unsigned* b, int n, unsigned* both, unsigned* either, double* similarity,
                            hipStream_t s) {
    const int per_block = FP_THREADS / 64;
    hipLaunchKernelGGL(tanimoto_kernel, dim3((n + per_block - 1) / per_block), dim3(FP_THREADS), 0, s, a, b, n, both, either, similarity);
    return hipGetLastError();
}

}  // namespace mnx
