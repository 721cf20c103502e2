// nearest.hip — for every query row of fingerprints the k nearest rows of a library by Tanimoto similarity (mnx_tanimoto_search):
// the search that mnx_tanimoto, pair by pair, is not. The rule stands in include/molnextr_hip.h ("Nearest rows"); the order is
// total, so the result does not depend on the grid, on the split into lists or on which wave arrives first. Two launches:
//   scan    grid (lists, query tiles). A workgroup keeps NEAREST_QUERY_TILE query rows and their bit counts in LDS and walks the
//           slabs w, w + lists, .. of NEAREST_SLAB_ROWS library rows. A thread holds one library row in 64 registers (sixteen
//           16-byte loads at the lane's own stride) and counts popcount(Q & R) against every query of the tile: the query words
//           are LDS reads of one address in all lanes, the count is the count-and-add form of the popcount; either = bits(Q) +
//           bits(R) - both. The counts cross the workgroup through LDS once per slab; then wave v keeps the lists of the queries
//           v, v + 4, .. of the tile — slot i of a list in lane i, in registers, for all the slabs — and takes in what beats a
//           list's k-th entry, one candidate of a wave ballot at a time. One list per (query, workgroup) goes to `work`.
//   merge   a wave per query: the lists of that query, each sorted, into one (nearest_select.h's merge, slot i in lane i), one
//           correctly rounded division per kept row, the cut at min_similarity, the output rows written whole.
// No atomic anywhere, global or LDS; nothing is allocated. Row offsets are size_t: nl * 256 bytes passes 4 GiB.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/molnextr_hip.h"
#include "nearest_select.h"
#include "table_passes.h"

namespace mnx {

namespace {

using nearest::entry;

constexpr int NS_THREADS = 256, NS_WAVES = NS_THREADS / 64;
constexpr int NS_TILE = MNX_NEAREST_QUERY_TILE, NS_SLAB = MNX_NEAREST_SLAB_ROWS;
constexpr int NS_OWN = NS_TILE / NS_WAVES;                  // the lists a wave keeps
constexpr int NS_CHUNKS = MNX_FP_WORDS / 4;                 // a row as 16-byte vectors
constexpr int NS_GROUP = 2;                                 // 16-byte vectors of a query read ahead of their use
constexpr unsigned NS_FILL_GROUPS = 1024;                   // workgroups that fill the chip: 256 CUs, 4 on each

static_assert(MNX_FP_WORDS == 64 && MNX_NEAREST_MAX_K == 64, "a list of k <= 64 slots is a wave of 64 lanes");
static_assert(NS_SLAB == NS_THREADS, "a thread per row of a slab");
static_assert(NS_TILE % NS_WAVES == 0, "the tile's lists are dealt to the waves");
static_assert(MNX_NEAREST_MAX_LISTS * MNX_NEAREST_SLAB_ROWS <= 131072, "the bound of the header");
static_assert(MNX_NEAREST_NONE == nearest::NONE, "one meaning, one value");

typedef unsigned row_vec __attribute__((ext_vector_type(4), aligned(4)));     // a caller's rows are 4-byte aligned, no more

// c into the wave's sorted list, slot i in lane i: nearest::insert with the position from one ballot
__device__ __forceinline__ void wave_insert(entry& mine, int lane, entry c) {
    const unsigned pos = (unsigned)__popcll(__ballot(nearest::before(mine, c)));      // the entries before c are a prefix
    const entry prev = __shfl_up(mine, 1, 64);
    mine = nearest::slot_after((unsigned)lane, pos, mine, prev, c);
}

__global__ __launch_bounds__(NS_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void nearest_scan_kernel(
        const unsigned* __restrict__ queries, int nq, const unsigned* __restrict__ library, unsigned nl, unsigned k, unsigned skip_self,
        unsigned n_slabs, unsigned n_lists, entry* __restrict__ work) {
    __shared__ uint4 q_words[NS_TILE][NS_CHUNKS];           // the tile's query rows
    __shared__ unsigned short q_bits[NS_TILE];              // their bit counts
    __shared__ unsigned short r_bits[NS_SLAB];              // the slab's rows' bit counts
    __shared__ unsigned short both[NS_TILE][NS_SLAB];       // popcount(Q & R) of the slab
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = blockIdx.y * NS_TILE, tq = min(NS_TILE, nq - q0);

    // ---- the tile: a thread per word, then a thread per query counts its bits ----
    for (int i = tid; i < tq * (int)MNX_FP_WORDS; i += NS_THREADS)
        ((unsigned*)q_words)[i] = queries[(size_t)q0 * MNX_FP_WORDS + i];
    __syncthreads();
    if (tid < tq) {
        unsigned n = 0;
        for (int w = 0; w < (int)MNX_FP_WORDS; ++w) n += (unsigned)__popc(((const unsigned*)q_words[tid])[w]);
        q_bits[tid] = (unsigned short)n;
    }

    entry list[NS_OWN];                                     // slot `lane` of the lists of queries wave, wave + 4, ..
#pragma unroll
    for (int o = 0; o < NS_OWN; ++o) list[o] = nearest::EMPTY;

    for (unsigned slab = blockIdx.x; slab < n_slabs; slab += n_lists) {
        const unsigned base = slab * (unsigned)NS_SLAB, row = base + (unsigned)tid;       // below 2^24 + 256
        // ---- this thread's row, in registers ----
        row_vec r[NS_CHUNKS];
        if (row < nl) {
            const row_vec* src = (const row_vec*)(library + (size_t)row * MNX_FP_WORDS);
#pragma unroll
            for (int c = 0; c < NS_CHUNKS; ++c) r[c] = src[c];
        } else {
#pragma unroll
            for (int c = 0; c < NS_CHUNKS; ++c) r[c] = row_vec{0u, 0u, 0u, 0u};
        }
        unsigned n = 0;
#pragma unroll
        for (int c = 0; c < NS_CHUNKS; ++c) n = __popc(r[c].x) + __popc(r[c].y) + __popc(r[c].z) + __popc(r[c].w) + n;
        __syncthreads();                                    // the last slab's counts have been read (and q_bits written)
        r_bits[tid] = (unsigned short)n;
        // ---- against every query of the tile: the words from LDS, one address in all lanes ----
#pragma unroll 1
        for (int q = 0; q < tq; ++q) {                      // one query at a time: 64 registers are the row's
            unsigned acc = 0;
            uint4 w[2][NS_GROUP];                           // the group in hand and the next one: no more query words in flight
#pragma unroll
            for (int c = 0; c < NS_GROUP; ++c) w[0][c] = q_words[q][c];
#pragma unroll
            for (int g = 0; g < NS_CHUNKS / NS_GROUP; ++g) {
                if (g + 1 < NS_CHUNKS / NS_GROUP) {
#pragma unroll
                    for (int c = 0; c < NS_GROUP; ++c) w[(g + 1) & 1][c] = q_words[q][(g + 1) * NS_GROUP + c];
                }
#pragma unroll
                for (int c = 0; c < NS_GROUP; ++c) {
                    const uint4 x = w[g & 1][c];
                    const row_vec y = r[g * NS_GROUP + c];
                    acc = __popc(x.x & y.x) + acc;
                    acc = __popc(x.y & y.y) + acc;
                    acc = __popc(x.z & y.z) + acc;
                    acc = __popc(x.w & y.w) + acc;
                }
                __builtin_amdgcn_sched_barrier(0);          // the scheduler would otherwise read all 64 words ahead, and spill the row
            }
            both[q][tid] = (unsigned short)acc;
        }
        __syncthreads();
        // ---- the wave's own lists take in what beats their k-th entry ----
#pragma unroll
        for (int o = 0; o < NS_OWN; ++o) {
            const int q = o * NS_WAVES + wave;              // uniform in the wave
            if (q >= tq) continue;
            const unsigned bits_q = q_bits[q], self = skip_self ? (unsigned)(q0 + q) : nearest::NONE;
            entry last = __shfl(list[o], (int)k - 1, 64);
            for (int part = 0; part < NS_SLAB / 64; ++part) {
                const int t = part * 64 + lane;
                const unsigned idx = base + (unsigned)t, n_and = both[q][t];
                const entry c = nearest::pack(n_and, bits_q + r_bits[t] - n_and, idx);
                bool open = idx < nl && idx != self && nearest::before(c, last);
                for (unsigned long long m = __ballot(open); m; m = __ballot(open)) {
                    const int from = __ffsll(m) - 1;
                    wave_insert(list[o], lane, __shfl(c, from, 64));
                    last = __shfl(list[o], (int)k - 1, 64);
                    open = open && lane != from && nearest::before(c, last);
                }
            }
        }
    }

    // ---- one list per (query, workgroup): slot i from lane i ----
#pragma unroll
    for (int o = 0; o < NS_OWN; ++o) {
        const int q = o * NS_WAVES + wave;
        if (q < tq && lane < (int)k) work[((size_t)(q0 + q) * n_lists + blockIdx.x) * k + lane] = list[o];
    }
}

__global__ __launch_bounds__(64) void nearest_merge_kernel(
        const entry* __restrict__ work, unsigned n_lists, unsigned k, double min_similarity, unsigned* __restrict__ count,
        unsigned* __restrict__ index, unsigned* __restrict__ both, unsigned* __restrict__ either, double* __restrict__ similarity) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const entry* lists = work + (size_t)q * n_lists * k;
    entry mine = nearest::EMPTY;
    for (unsigned w = 0; w < n_lists; ++w) {                // nearest::merge, the candidates of a list one ballot at a time
        const entry c = lane < (int)k ? lists[(size_t)w * k + lane] : nearest::EMPTY;
        entry last = __shfl(mine, (int)k - 1, 64);
        bool open = nearest::before(c, last);
        for (unsigned long long m = __ballot(open); m; m = __ballot(open)) {
            const int from = __ffsll(m) - 1;
            wave_insert(mine, lane, __shfl(c, from, 64));
            last = __shfl(mine, (int)k - 1, 64);
            open = open && lane != from && nearest::before(c, last);
        }
    }
    const unsigned idx = nearest::entry_index(mine), n_and = nearest::entry_both(mine), n_or = nearest::entry_either(mine);
    const double s = n_or ? (double)n_and / (double)n_or : 0.0;                         // one correctly rounded division
    const bool kept = lane < (int)k && idx != nearest::NONE && s >= min_similarity;      // a prefix: the list is sorted by s
    const unsigned n_kept = (unsigned)__popcll(__ballot(kept));
    if (lane == 0) count[q] = n_kept;
    if (lane < (int)k) {
        const size_t at = (size_t)q * k + lane;
        index[at] = kept ? idx : nearest::NONE;
        if (both) both[at] = kept ? n_and : 0u;
        if (either) either[at] = kept ? n_or : 0u;
        if (similarity) similarity[at] = kept ? s : 0.0;
    }
}

}  // namespace

// The lists per query: enough workgroups to fill the chip (NS_FILL_GROUPS over all query tiles), no more than there are slabs, no
// more than MNX_NEAREST_MAX_LISTS. With many queries a workgroup walks many slabs, and its lists soon refuse nearly every row.
static unsigned nearest_lists(int nq, unsigned nl) {
    const unsigned tiles = ((unsigned)nq + NS_TILE - 1) / NS_TILE, slabs = (nl + NS_SLAB - 1) / NS_SLAB;
    return std::min(std::min((NS_FILL_GROUPS + tiles - 1) / tiles, slabs), (unsigned)MNX_NEAREST_MAX_LISTS);
}

// 8 k min(nq min(MAX_LISTS, slabs), 32768 + nq): above nq * nearest_lists * k entries (nq / tiles <= NS_TILE), and monotone
size_t tanimoto_search_work_bytes(int nq, unsigned nl, unsigned k) {
    const size_t slabs = ((size_t)nl + NS_SLAB - 1) / NS_SLAB;
    return sizeof(entry) * k * std::min((size_t)nq * std::min((size_t)MNX_NEAREST_MAX_LISTS, slabs), (size_t)NS_FILL_GROUPS * NS_TILE + (size_t)nq);
}

hipError_t tanimoto_search_enqueue(const unsigned* queries, int nq, const unsigned* library, unsigned nl, unsigned k,
                                   double min_similarity, unsigned flags, unsigned* count, unsigned* index, unsigned* both,
                                   unsigned* either, double* similarity, void* work, hipStream_t s) {
    const unsigned tiles = ((unsigned)nq + NS_TILE - 1) / NS_TILE, slabs = (nl + NS_SLAB - 1) / NS_SLAB, lists = nearest_lists(nq, nl);
    hipLaunchKernelGGL(nearest_scan_kernel, dim3(lists, tiles), dim3(NS_THREADS), 0, s, queries, nq, library, nl, k,
                       flags & MNX_NEAREST_SKIP_SELF, slabs, lists, (entry*)work);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(nearest_merge_kernel, dim3(nq), dim3(64), 0, s, (const entry*)work, lists, k, min_similarity, count, index,
                       both, either, similarity);
    return hipGetLastError();
}

}  // namespace mnx
