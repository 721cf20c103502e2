// gemm256.hip — the persistent large-tile form of the encoder GEMM for its 16-bit-output layers (qkv: bias, fc1: bias +
// GELU): C = epi(A.W^T + b), A [M,K], W [N,K] 16-bit, K contiguous; M and N multiples of 256, K a multiple of 64, >= 128.
// launch_gemm16 (gemm.hip) routes here when gemm256_supports() says so; every other shape / epilogue stays on the
// 128x128 kernel of gemm.hip.
//
// Why a second kernel (measurements: profiles/r02_gemm_shapes.md):
//   * the 128x128 kernel moves 32 KiB through the L2 -> LDS fill path per 2.1 MFLOP K-step (64 FLOP/B); a CU issues
//     4096 bf16 FLOP/clk but its fill path carries ~64 B/clk, so that tile saturates the fill path where the matrix
//     pipe would saturate. A 256x256 tile needs half the bytes per FLOP;
//   * with K = 256..1024 a tile is only 4..16 K-steps: prologue (first loads), epilogue (convert + store 128 KiB) and
//     the GELU arithmetic were as long as the K loop and ran strictly after it. Here they overlap.
//
// Structure (gfx950, one 512-thread workgroup per CU, grid = min(tiles, 256), tile t -> workgroup t mod grid):
//   * 256x256 output tile, 8 waves as 2 (M) x 4 (N), each wave 128x64 = 8x4 MFMA 16x16x32 tiles (128 accumulator
//     registers), MFMA issued "swapped" so a lane owns 4 consecutive output columns of a row (as gemm.hip);
//   * BK = 64. A K-tile lives in LDS as FOUR 16 KiB slots: Am0 / Am1 = the first / second 64 rows of each wave-row
//     block, Bn0 / Bn1 = the first / second 32 weight rows of each wave-column block. Two K-tile buffers = 8 slots =
//     128 KiB. Each slot is a [128][64] 16-bit image with the XOR swizzle of gemm.hip (conflict-free ds_read_b128),
//     filled by global_load_lds_dwordx4 (2 per thread, scalar base + 32-bit lane offset);
//   * a K-tile is TWO phases of 32 MFMAs per wave: phase A reads Am0 + Bn0 + Bn1 (16 ds_read_b128) and issues the fill
//     of Am1 of the next K-tile; phase B reads Am1 (8) and issues the fills of Am0 + Bn0 + Bn1 of the K-tile after.
//     Four slot-fills are in flight at every wait, retired with counted vmcnt (never 0 inside the stream);
//   * the two wave rows (waves w and w+4 share a SIMD) run half a phase apart: one row's MFMAs cover the other row's
//     LDS reads, waits and fill issue (one raw s_barrier before and one after each MFMA block);
//   * the workgroup is persistent: the K-tile ring streams through all of its tiles without draining, so the first
//     K-tiles of the next tile are loading while the finished tile is converted and stored;
//   * epilogue: each wave transposes its 128x64 accumulator tile in 16-row slabs through a PRIVATE 2 KiB LDS patch (no
//     workgroup barrier) and stores whole 128-byte lines, 16 bytes per lane. The second wave row runs its epilogue
//     before its closing barrier, the first row after its own, so both run concurrently (measured: placed the same way
//     for both rows, each row held the other at a barrier and the two epilogues ran one after the other);
//   * GELU is gelu_fast4 (common.h): 17 fp32 operations per value. It remains exposed: the matrix pipe idles while the
//     VALU converts (5-7 us of a ~20 us fc1 tile at K = 512).
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace mnx {

namespace {

typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void glb_void_t;

constexpr int TM = 256, TN = 256, TK = 64;
constexpr int SLOT = 128 * TK * 2;            // 16 KiB

__device__ __forceinline__ int lds_off256(int r, int c) { return r * 128 + ((c ^ ((r >> 1) & 7)) << 4); }

template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// vmcnt bookkeeping (loads and stores retire in issue order): per tile a wave issues, besides the fills, 4 bias loads
// (inline asm, at the tile's first K-tile) and 16 stores (epilogue). A wait that retires a fill issued BEFORE those
// operations must allow them as younger operations; the exact counts are derived at each wait in the kernel. A count
// that is too small only stalls, one that is too large would read a slot before it has landed.
constexpr int P_STG = 2048;                        // per-wave staging patch: 16 rows x 64 columns of a 16-bit type
constexpr int P_LDS = 8 * SLOT + 8 * P_STG;        // 144 KiB
constexpr int P_STORES = 16, P_BIAS = 4;           // VMEM operations per wave per tile besides the fills

// SPLIT (kernels.h SplitArgs, dtypes BF16X3 / F16X3) with terms == 1 (the error-budget aid): only the hi planes are
// multiplied, the epilogue computes epi(oscale * acc + bias) with the exact-erf GELU and stores TWO planes (hi, lo):
// 2 x P_STORES stores per wave per tile. All three terms: gemm256x3_kernel below.
template <typename T, int EPI, bool SPLIT>
__global__ __launch_bounds__(512) void gemm256_kernel(const T* __restrict__ A, const T* __restrict__ W, T* __restrict__ C,
                                                       const float* __restrict__ bias, int M, int N, int K, int tiles_n,
                                                       int n_tiles, const SplitArgs sp) {
    static_assert(EPI == EPI_BIAS_16 || EPI == EPI_GELU_16, "persistent form: 16-bit outputs only");
    typedef typename H16<T>::v8 v8;
    typedef typename H16<T>::v4 v4;
    constexpr int PST = SPLIT ? 2 * P_STORES : P_STORES;          // stores per wave per tile
    extern __shared__ __attribute__((aligned(16))) char smem[];     // 8 ring slots of 16 KiB + 8 staging patches
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int fr = lane & 15, fg = lane >> 4;
    const int nk = K / TK, nkk = nk;
    const int my_first = blockIdx.x, stride = gridDim.x;
    const int my_tiles = (n_tiles - my_first + stride - 1) / stride;
    const int total_kt = my_tiles * nkk;                  // K-tiles this workgroup streams through the ring

    // per-thread byte offsets of its two DMA pieces inside a tile (tile origin and K offset live in scalar registers)
    const int r_in = lane >> 3, pc = lane & 7;
    unsigned offA[2][2], offB[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int s = (wave * 2 + i) * 8 + r_in;
        const int sw = (pc ^ ((s >> 1) & 7)) << 3;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            offA[h][i] = (unsigned)((((s >> 6) * 128 + h * 64 + (s & 63)) * K + sw) * 2);
            offB[h][i] = (unsigned)((((s >> 5) * 64 + h * 32 + (s & 31)) * K + sw) * 2);
        }
    }
    // the fill stream's position: K-tile `f` (slots 0..2 are issued two K-tiles ahead, slot 3 one K-tile ahead)
    struct Pos { const char* a; const char* w; int kt, seq; };
    auto tile_origin = [&](int seq, int& m0, int& n0) {
        const int tile = xcd_remap(my_first + seq * stride, n_tiles);
        m0 = (tile / tiles_n) * TM; n0 = (tile % tiles_n) * TN;
    };
    auto pos_at = [&](int seq) {
        int m0, n0; tile_origin(seq, m0, n0);
        Pos q; q.a = (const char*)(A + (size_t)m0 * K); q.w = (const char*)(W + (size_t)n0 * K); q.kt = 0; q.seq = seq;
        return q;
    };
    auto advance = [&](Pos& q) {
        if (++q.kt == nk) { if (q.seq + 1 < my_tiles) q = pos_at(q.seq + 1); else { q.kt = 0; ++q.seq; } }
        else { q.a += TK * 2; q.w += TK * 2; }
    };
    auto fill = [&](const Pos& q, int par, auto slot_c) {
        constexpr int sl = decltype(slot_c)::value;
        char* dst = smem + (par * 4 + sl) * SLOT;
        const char* base = (sl == 0 || sl == 3) ? q.a : q.w;
        const unsigned o0 = sl == 0 ? offA[0][0] : sl == 1 ? offB[0][0] : sl == 2 ? offB[1][0] : offA[1][0];
        const unsigned o1 = sl == 0 ? offA[0][1] : sl == 1 ? offB[0][1] : sl == 2 ? offB[1][1] : offA[1][1];
        __builtin_amdgcn_global_load_lds((glb_void_t*)(base + o0), (lds_void_t*)(dst + (wave * 2) * 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((glb_void_t*)(base + o1), (lds_void_t*)(dst + (wave * 2 + 1) * 1024), 16, 0, 0);
    };
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;
    using S2 = std::integral_constant<int, 2>;
    using S3 = std::integral_constant<int, 3>;

    // bias of the tile being accumulated: 4 x 4 columns per lane, loaded by inline asm so that the loads are retired by
    // the counted waits of the main loop (a compiler-tracked load would drain the whole ring at its first use)
    // (the compiler believes b4 is valid right after the asm statement: nothing may read or copy it before the waits of
    //  the following K-tile have retired the loads — its only readers are in the epilogue, many waits later; the
    //  all-element test tests/test_gpu_parity.py::test_gemm_persistent_256_tile_kernel guards this against a compiler
    //  that would split the live range)
    f32x4 b4[4];
    auto load_bias = [&](int n0) {
        const float* bp = bias + n0 + wc * 64 + fg * 4;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
            asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(b4[nt]) : "v"(bp + nt * 16) : "memory");
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    int m0, n0;
    tile_origin(0, m0, n0);
    load_bias(n0);
    Pos p1 = pos_at(0);                           // K-tile gk + 1 (slot 3)
    Pos p2 = p1;                                  // K-tile gk + 2 (slots 0..2)
    fill(p1, 0, S0{}); fill(p1, 0, S1{}); fill(p1, 0, S2{}); fill(p1, 0, S3{});
    advance(p1); p2 = p1;
    fill(p2, 1, S0{}); fill(p2, 1, S1{}); fill(p2, 1, S2{});
    advance(p2);
    wait_vm<8>();                                 // bias + Am0, Bn0, Bn1 of K-tile 0 (Am1(0) and K-tile 1's three may fly)
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();    // second wave row starts one segment late

    char* stg = smem + 8 * SLOT + wave * P_STG;
    v8 af[4][2], b0[2][2], b1[2][2];
    int kt = 0, seq = 0;
    auto epilogue = [&]() {
        // ---- epilogue of tile `seq`: 16-row slabs of the wave tile through the wave's own staging patch ----
        // b4 was written by untracked loads at the tile's first K-tile; every counted wait since then has retired them (they
        // are older than the fills those waits cover). The empty asm is the point from which the compiler may read b4: it
        // cannot hoist, copy or rematerialise a use above it.
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) asm volatile("" : "+v"(b4[nt]));
        T* crow = C + (size_t)(m0 + wr * 128 + (lane >> 3)) * N + n0 + wc * 64 + (lane & 7) * 8;
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
            v4 lo[4];                                   // SPLIT: the slab's lo plane, derived together with hi (common.h split16)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                v4 o4;
                if (SPLIT) {
                    f32x4 v = acc[mt][nt] * sp.oscale + b4[nt];
                    if (EPI == EPI_GELU_16) v = gelu_split4(v);
                    split16x4<T>(v, o4, lo[nt]);
                } else {
                    f32x4 v = acc[mt][nt] + b4[nt];
                    if (EPI == EPI_GELU_16) v = gelu_fast4(v);
                    o4 = (v4){(T)v[0], (T)v[1], (T)v[2], (T)v[3]};
                }
                acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
                *(v4*)(stg + fr * 128 + (((nt * 2 + (fg >> 1)) ^ (fr & 7)) << 4) + (fg & 1) * 8) = o4;
            }
            // the wave's LDS operations execute in order: the reads below see the slab, the next slab's writes
            // follow these reads
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int row = (lane >> 3) + 8 * i;
                const v8 o8 = *(const v8*)(stg + row * 128 + (((lane & 7) ^ (row & 7)) << 4));
                *(v8*)(crow + (size_t)(mt * 16 + 8 * i) * N) = o8;
            }
            if (SPLIT) {
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
                    *(v4*)(stg + fr * 128 + (((nt * 2 + (fg >> 1)) ^ (fr & 7)) << 4) + (fg & 1) * 8) = lo[nt];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int row = (lane >> 3) + 8 * i;
                    const v8 o8 = *(const v8*)(stg + row * 128 + (((lane & 7) ^ (row & 7)) << 4));
                    *(v8*)(crow + sp.c_lo + (size_t)(mt * 16 + 8 * i) * N) = o8;
                }
            }
        }
    };
    for (int gk = 0; gk < total_kt; ++gk) {
        const bool last_kt = (kt == nkk - 1);
        const char* buf = smem + (gk & 1) * 4 * SLOT;
        const bool tail = gk + 2 >= total_kt;     // the ring is running dry: drain instead of counting
        const bool first_kt = (kt == 0 && seq > 0), second_kt = (kt == 1 && seq > 0);
        // ---- phase A: Am0 + Bn0 + Bn1 -> rows 0..63 of the wave tile ----
        if (gk + 1 < total_kt) fill(p1, (gk + 1) & 1, S3{});
        if (first_kt) load_bias(n0);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                b0[j][ks] = *(const v8*)(buf + 1 * SLOT + lds_off256(wc * 32 + j * 16 + fr, ks * 4 + fg));
                b1[j][ks] = *(const v8*)(buf + 2 * SLOT + lds_off256(wc * 32 + j * 16 + fr, ks * 4 + fg));
            }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                af[i][ks] = *(const v8*)(buf + 0 * SLOT + lds_off256(wr * 64 + i * 16 + fr, ks * 4 + fg));
        // Am1 of this K-tile, issued in phase A of the previous one. Younger: the 3 fills of phase B(gk-1), [the 16
        // stores of the epilogue], this phase's fill [+ 4 bias loads]; after a tile's first K-tile the bias loads of
        // that K-tile are younger than the fill issued just before them.
        if (tail) wait_vm<0>();
        else if (first_kt) wait_vm<8 + PST + P_BIAS>();
        else if (second_kt) wait_vm<8 + P_BIAS>();
        else wait_vm<8>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[i][j] = H16<T>::mfma(b0[j][ks], af[i][ks], acc[i][j]);
                    acc[i][2 + j] = H16<T>::mfma(b1[j][ks], af[i][ks], acc[i][2 + j]);
                }
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_s_barrier();
        // ---- phase B: Am1 -> rows 64..127 ----
        if (gk + 2 < total_kt) { fill(p2, gk & 1, S0{}); fill(p2, gk & 1, S1{}); fill(p2, gk & 1, S2{}); }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                af[i][ks] = *(const v8*)(buf + 3 * SLOT + lds_off256(wr * 64 + i * 16 + fr, ks * 4 + fg));
        // Am0, Bn0, Bn1 of the next K-tile, issued in phase B of the previous one. Younger: [16 stores], the fill of
        // phase A(gk) [+ 4 bias loads], this phase's three fills.
        if (tail) wait_vm<0>();
        else if (first_kt) wait_vm<8 + PST + P_BIAS>();
        else wait_vm<8>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[4 + i][j] = H16<T>::mfma(b0[j][ks], af[i][ks], acc[4 + i][j]);
                    acc[4 + i][2 + j] = H16<T>::mfma(b1[j][ks], af[i][ks], acc[4 + i][2 + j]);
                }
        __builtin_amdgcn_s_setprio(0);
        // The tile's epilogue has no barrier of its own. The second wave row runs it BEFORE its closing barrier (which
        // pairs with the first row's next opening barrier), the first row AFTER its own: both rows then convert and
        // store at the same time instead of one after the other (each would otherwise hold the other at a barrier).
        if (last_kt && wr == 1) epilogue();
        __builtin_amdgcn_s_barrier();
        if (last_kt && wr == 0) epilogue();
        p1 = p2;
        advance(p2);
        if (last_kt) {
            kt = 0; ++seq;
            if (seq < my_tiles) tile_origin(seq, m0, n0);
        } else {
            ++kt;
        }
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();    // the first wave row waits for the second one's last segment
}

// =====================================================================================================================
// gemm256x3_kernel — the split-operand form (dtypes BF16X3 / F16X3) with all THREE product terms (SplitArgs::terms == 3:
// ah.wl + ah.wh + al.wh) or with TWO (terms == 2: ah.wl + ah.wh — the activation's lo plane is neither read nor multiplied;
// the weight keeps both planes. compute_dtype FP16X3M runs the op classes on two terms whose error budget allows it).
//
// THREE TERMS. Streaming the three terms of a K-tile as three complete K-tiles costs 12 slot fills and 72 fragment reads per
// 192 MFMAs of a wave, although A hi and W hi are each needed twice. This kernel keeps the four operand slabs of ONE K-tile
// resident — the 8 ring slots are A hi (2), A lo (2), W hi (2), W lo (2) — and walks the six 32-MFMA products of the tile in
// an order in which consecutive products share one register operand:
//
//     phase  product      fragments read (LDS)            slot refilled at the START of the phase (read last in the
//                                                          phase before)                       wait for (next phase)
//     P1     Ah0 . Wl     Ah0 (8) + Wl (8)                A lo, rows 64-127 of THIS K-tile       Ah1
//     P2     Ah1 . Wl     Ah1 (8)  [Wl stays in regs]     W lo (both halves) of the NEXT K-tile   Wh
//     P3     Ah1 . Wh     Wh (8)   [Ah1 stays]            A hi, rows 64-127 of the next          —  (Ah0 landed before P1)
//     P4     Ah0 . Wh     Ah0 (8)  [Wh stays]             W hi (both halves) of the next          Al0
//     P5     Al0 . Wh     Al0 (8)  [Wh stays]             A hi, rows 0-63   of the next          Al1
//     P6     Al1 . Wh     Al1 (8)  [Wh stays]             A lo, rows 0-63   of the next          Ah0', Wl' of the next
//
// (rows = the first / second 64 rows of each wave-row block, as the Am0 / Am1 slots of gemm256_kernel; the W slots are its
// Bn0 / Bn1.) 8 slot fills and 56 fragment reads per 192 MFMAs. EVERY output element accumulates its terms in the order
// hi.lo, hi.hi, lo.hi within a K-tile — the order of the 128x128 kernel's three-term schedule (gemm.hip) — so that the two
// kernels, between which launch_gemm16 splits a layer's rows by batch size, add the same fp32 numbers in the same order:
// an image's features do not depend on the batch it is encoded in. (Chaining the phases by register reuse alone would
// give the two row halves different orders — a uniform order costs one repeated fragment read, Ah0 in P1 and P4.)
// Every slot is single-buffered: it is refilled in the phase after its last read and needed again 5 phases later —
// except A hi rows 0-63 (read in P1 and P4, refilled in P5, needed in P1: 2 phases).
//
// TWO TERMS: phases P1-P4 of the table are the whole K-tile (order hi.lo, hi.hi for every row, again the 128x128 kernel's).
// 6 slot fills and 40 fragment reads per 128 MFMAs. A hi rows 0-63 is read in the first AND the last phase of a K-tile, so it
// alternates between two slots by K-tile parity (slot 0 and the A lo slot 2, free in this form): the next K-tile's copy is
// requested in P1 (4 phases of lead); W lo is refilled in P2, A hi rows 64-127 in P3, W hi in P4 (3 phases of lead each).
//
// Phase skeleton, barrier pairing of the two wave rows (half a phase apart) and the epilogue are those of gemm256_kernel:
// a slot read in phase n may be overwritten from the start of phase n + 1 (the other row passed its opening barrier of
// phase n, after its reads); data read in phase n + 1 is waited for (counted vmcnt) before the opening barrier of phase n.
// vmcnt: a wave issues 16 fill instructions per K-tile in the order P1: 2, P2: 4, P3: 2, P4: 4, P5: 2, P6: 2 (two terms: 12 —
// P1: 2, P2: 4, P3: 2, P4: 4); the number of younger operations allowed at each wait is derived below. First K-tile of the
// stream and last K-tile of the stream (different in-flight population) drain instead of counting.
// (dma16 / dma4, the LDS-DMA helpers every fill of this kernel goes through, live in common.h.)
//
// LO_OUT (16-bit epilogues): write the output's lo plane too. false when the consumer runs on two terms (fc1 -> fc2 in
// FP16X3M): half the epilogue's stores, and the hi plane is bit-identical to the one the two-plane form writes.
//
// The fp32-output epilogue (bias [+ in-place residual] -> fp32) is hand-issued: residual loads and stores are inline asm on
// ONE scalar base + a 32-bit lane offset, retired by counted vmcnt — four 16-row slabs of residual in flight per wave (the
// registers are the main loop's dead operand fragments), stores never waited for —, every access a whole 128-byte line: the
// slab goes through the wave's staging patch in two 32-column halves into the row-major lane mapping of the 16-bit epilogue
// (8 rows x 128 B per instruction), the residual is loaded in that mapping directly. (DESIGN.md "fp32-output epilogue";
// the two earlier forms — compiler-tracked loads / stores, and counted loads in the accumulator mapping — and the loop
// ablation hooks of round 5 are in git history at 7f4ab81, their measurements in profiles/r05_gemm_lab_*.txt.)

constexpr int X3_BIAS = 1;                                 // one 4-byte-per-lane DMA per wave per tile (its 64 bias values)
constexpr int X3_LDS = P_LDS + 8 * 256;                    // + a 256-byte bias patch per wave

// Effective shader clock of the launches (measurement aid, always compiled): workgroup 0 adds its lifetime in shader cycles
// (s_memtime) and in 100 MHz ticks (s_memrealtime) to two counters; x3_clock_read() turns them into MHz. The chip clocks to
// its power budget — 1.65-1.9 GHz under this kernel with real operands, 2.39 GHz on zeros (profiles/r05_gemm_lab_ablations.txt)
// — so a rate only means something next to the clock it was reached at. Cost: four scalar instructions per launch.
__device__ unsigned long long x3_clk_acc[2];

// fp32 epilogue: vector-memory operations younger than the residual loads of slab mt when they are waited for
// (4 loads + 4 stores per slab, four slabs of loads in flight): 12 16 20 24 24 20 16 12
__device__ __forceinline__ void x3_wait_younger(int mt) {
    const int y = mt < 4 ? 12 + 4 * mt : 12 + 4 * (7 - mt);
    switch (y) {
        case 12: wait_vm<12>(); break;
        case 16: wait_vm<16>(); break;
        case 20: wait_vm<20>(); break;
        default: wait_vm<24>(); break;
    }
}

template <typename T, int EPI, int TERMS, bool LO_OUT>
__global__ __launch_bounds__(512) void gemm256x3_kernel(const T* __restrict__ A, const T* __restrict__ W, void* Cv,
                                                         const float* __restrict__ bias, const float* resid, int M, int N,
                                                         int K, int tiles_n, int n_tiles, const SplitArgs sp) {
    static_assert(TERMS == 2 || TERMS == 3, "two or three product terms");
    typedef typename H16<T>::v8 v8;
    typedef typename H16<T>::v4 v4;
    constexpr bool OUT16 = (EPI == EPI_BIAS_16 || EPI == EPI_GELU_16);
    static_assert(OUT16 || LO_OUT, "LO_OUT only distinguishes the 16-bit epilogues");
    // vector-memory operations of a tile's epilogue per wave: 16 stores per 16-bit plane; fp32 output 32 stores
    // (+ 32 residual loads)
    constexpr int PST = OUT16 ? (LO_OUT ? 2 : 1) * P_STORES : (EPI == EPI_RESID_F32 ? 64 : 32);
    T* C = (T*)Cv;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int fr = lane & 15, fg = lane >> 4;
    const int nk = K / TK;
    const int my_first = blockIdx.x, stride = gridDim.x;
    const int my_tiles = (n_tiles - my_first + stride - 1) / stride;
    const int total_kt = my_tiles * nk;
    const long a_lo_b = (long)sp.a_lo * 2, w_lo_b = (long)sp.w_lo * 2;
    enum { S_AH0 = 0, S_AH1 = 1, S_AL0 = 2, S_AL1 = 3, S_WH0 = 4, S_WH1 = 5, S_WL0 = 6, S_WL1 = 7 };

    // DMA addressing: a wave fills two 1 KiB pieces (8 rows x 128 B) of every slot. The lane part of a piece's source
    // offset is the same for both 64-row halves of A (both 32-row halves of W): the half is a scalar addend on the base.
    const int r_in = lane >> 3, pc = lane & 7;
    unsigned offA[2], offB[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int s = (wave * 2 + i) * 8 + r_in;
        const int sw = (pc ^ ((s >> 1) & 7)) << 3;
        offA[i] = (unsigned)((((s >> 6) * 128 + (s & 63)) * K + sw) * 2);
        offB[i] = (unsigned)((((s >> 5) * 64 + (s & 31)) * K + sw) * 2);
    }
    const long halfA_b = (long)64 * K * 2, halfB_b = (long)32 * K * 2;
    const unsigned lds0 = (unsigned)(__UINTPTR_TYPE__)(lds_char_t*)smem + (unsigned)(wave * 2048);   // the wave's first piece of slot 0
    struct Pos { const char* a; const char* w; int kt, seq; };      // hi planes of one K-tile
    auto tile_origin = [&](int seq, int& m0, int& n0) {
        const int tile = xcd_remap(my_first + seq * stride, n_tiles);
        m0 = (tile / tiles_n) * TM; n0 = (tile % tiles_n) * TN;
    };
    auto pos_at = [&](int seq) {
        int m0, n0; tile_origin(seq, m0, n0);
        Pos q; q.a = (const char*)(A + (size_t)m0 * K); q.w = (const char*)(W + (size_t)n0 * K); q.kt = 0; q.seq = seq;
        return q;
    };
    auto advance = [&](Pos& q) {
        if (++q.kt == nk) { if (q.seq + 1 < my_tiles) q = pos_at(q.seq + 1); else { q.kt = 0; ++q.seq; } }
        else { q.a += TK * 2; q.w += TK * 2; }
    };
    auto fill_a = [&](const char* base, int half, int slot) {       // 64-row half of every wave-row block -> one slot
        const char* b = base + half * halfA_b;
        dma16(offA[0], b, lds0 + slot * SLOT);
        dma16(offA[1], b, lds0 + slot * SLOT + 1024);
    };
    auto fill_w = [&](const char* base, int slot0) {                // both 32-row halves of every wave-column block -> two slots
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const char* b = base + h * halfB_b;
            dma16(offB[0], b, lds0 + (slot0 + h) * SLOT);
            dma16(offB[1], b, lds0 + (slot0 + h) * SLOT + 1024);
        }
    };
    // bias of the tile being accumulated: the wave's 64 values, DMA'd into its own 256-byte LDS patch at the tile's first
    // K-tile (one more entry of the in-order vmcnt queue, retired by the counted waits) and read in the epilogue
    const float* bias_s = (const float*)(smem + P_LDS + wave * 256);
    const unsigned bias_lds = (unsigned)(__UINTPTR_TYPE__)(lds_char_t*)smem + (unsigned)(P_LDS + wave * 256);
    auto load_bias = [&](int n0) { dma4((unsigned)(lane * 4), (const char*)(bias + n0 + wc * 64), bias_lds); };
    // (a layer without bias — the patch-merging reduction — passes a zero vector: launch_gemm256x3 substitutes one)

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    unsigned long long clk_c0 = 0, clk_r0 = 0;
    if (blockIdx.x == 0) { clk_c0 = __builtin_readcyclecounter(); clk_r0 = __builtin_amdgcn_s_memrealtime(); }
    int m0, n0;
    tile_origin(0, m0, n0);
    load_bias(n0);
    Pos cur = pos_at(0);
    // prologue: everything K-tile 0 needs in the order of first use (three terms: except A lo rows 64-127, issued by its own
    // P1; A lo rows 0-63 last)
    fill_a(cur.a, 0, S_AH0); fill_w(cur.w + w_lo_b, S_WL0); fill_a(cur.a, 1, S_AH1); fill_w(cur.w, S_WH0);
    if (TERMS == 3) fill_a(cur.a + a_lo_b, 0, S_AL0);
    Pos nxt = cur;
    advance(nxt);
    if (TERMS == 3) wait_vm<8>();                 // bias, Ah0, W lo landed (Ah1 2 + W hi 4 + Al0 2 may fly)
    else wait_vm<6>();                            // bias, Ah0, W lo landed (Ah1 2 + W hi 4 may fly)
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();    // second wave row starts one segment late

    char* stg = smem + 8 * SLOT + wave * P_STG;
    v8 af[4][2], b0[2][2], b1[2][2];
    // fragment addresses: the swizzle term of lds_off256 depends on (row >> 1) & 7 = (fr >> 1) & 7 only, so the 16-row
    // tile index and the slot are immediate offsets on two lane-dependent bases per operand (one per 32-wide K half)
    const char* a_rd[2];
    const char* w_rd[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        a_rd[ks] = smem + lds_off256(wr * 64 + fr, ks * 4 + fg);
        w_rd[ks] = smem + S_WH0 * SLOT + lds_off256(wc * 32 + fr, ks * 4 + fg);
    }
    auto read_a_at = [&](int byte_off) {          // byte_off: slot * SLOT (an immediate when the slot is a constant)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) af[i][ks] = *(const v8*)(a_rd[ks] + byte_off + i * 2048);
    };
    auto read_a = [&](auto slot_c) { read_a_at(decltype(slot_c)::value * SLOT); };
    auto read_w = [&](auto slot_c) {
        constexpr int rel = decltype(slot_c)::value - S_WH0;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                b0[j][ks] = *(const v8*)(w_rd[ks] + rel * SLOT + j * 2048);
                b1[j][ks] = *(const v8*)(w_rd[ks] + (rel + 1) * SLOT + j * 2048);
            }
    };
    using R_AH0 = std::integral_constant<int, S_AH0>;
    using R_AH1 = std::integral_constant<int, S_AH1>;
    using R_AL0 = std::integral_constant<int, S_AL0>;
    using R_AL1 = std::integral_constant<int, S_AL1>;
    using R_WH = std::integral_constant<int, S_WH0>;
    using R_WL = std::integral_constant<int, S_WL0>;
    // the 32 MFMAs of one phase: rows [mb*16, mb*16 + 64) of the wave tile += af . (b0 | b1)
    auto mfma_block = [&](auto mb_c) {
        constexpr int mb = decltype(mb_c)::value;
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[mb + i][j] = H16<T>::mfma(b0[j][ks], af[i][ks], acc[mb + i][j]);
                    acc[mb + i][2 + j] = H16<T>::mfma(b1[j][ks], af[i][ks], acc[mb + i][2 + j]);
                }
        __builtin_amdgcn_s_setprio(0);
    };
    using MB0 = std::integral_constant<int, 0>;
    using MB4 = std::integral_constant<int, 4>;
    auto epilogue = [&]() {
        f32x4 b4[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) b4[nt] = *(const f32x4*)(bias_s + nt * 16 + fg * 4);
        if (!OUT16) {
            // ---- fp32 output (+ in-place fp32 residual). Residual loads and stores are inline asm on a scalar base (the wave's
            // 128 x 64 block of the tile) + a 32-bit lane offset; no compiler-tracked vector-memory operation exists in this
            // epilogue, so the compiler adds no wait of its own. In-order retirement: the sequence of a wave is
            // L0 L1 L2 L3 | S0 L4 | S1 L5 | S2 L6 | S3 L7 | S4 | S5 | S6 | S7 (L = 4 residual loads of a slab, S = its 4 stores);
            // the residual of slab mt is complete once at most x3_wait_younger(mt) younger operations are outstanding. Every
            // element is read and written by the same lane (C may alias the residual), and a slab's loads are issued after the
            // stores of the slab four before it, whose rows they do not touch.
            constexpr bool RES = (EPI == EPI_RESID_F32);
            // ONE scalar base per array for the whole epilogue; everything that changes from slab to slab is in the 32-bit lane
            // offset (a VALU result: its hand-over to a vector-memory instruction is interlocked by the hardware). Reason:
            // gfx950 requires wait states between a SALU write of an SGPR and a vector-memory instruction that uses it as its
            // address base, and the compiler's hazard recognizer does not look into inline asm — the first build of this
            // epilogue re-derived the base per slab with s_add / s_addc right in front of the asm stores and 1.4 % of the words
            // landed elsewhere. The s_nop below covers the one place where the bases are produced. The stores carry their own
            // s_nop: a VALU write of the data registers of a 16-byte store in the very next instruction is the other hazard
            // the compiler cannot see (0.2 % wrong words in the bias-only form). tests/test_device_math.py pins both in the ISA.
            const size_t wbase = ((size_t)(m0 + wr * 128) * N + n0 + wc * 64) * 4;
            const char* cb = (const char*)Cv + wbase;
            const char* rb = RES ? (const char*)resid + wbase : cb;
            asm volatile("s_nop 4" ::"s"(cb), "s"(rb));
            const unsigned slab_b = (unsigned)N * 64u;                // 16 rows
#define MNX_X3_LD1(dst, off, imm) asm volatile("global_load_dwordx4 %0, %1, %2 offset:" #imm : "=&v"(dst) : "v"(off), "s"(rb) : "memory")
#define MNX_X3_ST1(src, off, imm) asm volatile("global_store_dwordx4 %0, %1, %2 offset:" #imm "\n\ts_nop 1" ::"v"(off), "v"(src), "s"(cb) : "memory")
            // row-major mapping: lane l <-> row (l >> 3) (+ 8 for the second access), 16 bytes at column 4 (l & 7) of a
            // 32-column half: d[2 h + i] = rows 8 i .. 8 i + 7 of half h
            const unsigned voff = (unsigned)((((lane >> 3)) * N + (lane & 7) * 4) * 4);
            const unsigned half_b = (unsigned)N * 32u;                // 8 rows
#define MNX_X3_LD(d, mt)                                                                                                  \
    do {                                                                                                                  \
        const unsigned o_ = voff + (unsigned)(mt) * slab_b, o8_ = o_ + half_b;                                            \
        MNX_X3_LD1(d[0], o_, 0); MNX_X3_LD1(d[1], o8_, 0); MNX_X3_LD1(d[2], o_, 128); MNX_X3_LD1(d[3], o8_, 128);        \
    } while (0)
#define MNX_X3_ST(v, mt)                                                                                                  \
    do {                                                                                                                  \
        const unsigned o_ = voff + (unsigned)(mt) * slab_b, o8_ = o_ + half_b;                                            \
        MNX_X3_ST1(v[0], o_, 0); MNX_X3_ST1(v[1], o8_, 0); MNX_X3_ST1(v[2], o_, 128); MNX_X3_ST1(v[3], o8_, 128);        \
    } while (0)
            f32x4 r[4][4];
            if (RES) {
                MNX_X3_LD(r[0], 0); MNX_X3_LD(r[1], 1); MNX_X3_LD(r[2], 2); MNX_X3_LD(r[3], 3);
            }
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) {
                f32x4 v[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    v[nt] = acc[mt][nt] * sp.oscale + b4[nt];
                    acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
                }
                // accumulator mapping -> row-major mapping through the wave's staging patch, one 32-column half at a time
                // (16 rows x 128 B = the 2 KiB patch; a wave's LDS operations execute in order)
                f32x4 t[4];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
#pragma unroll
                    for (int q = 0; q < 2; ++q) *(f32x4*)(stg + fr * 128 + (((q * 4 + fg) ^ (fr & 7)) << 4)) = v[2 * h + q];
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int row = (lane >> 3) + 8 * i;
                        t[2 * h + i] = *(const f32x4*)(stg + row * 128 + (((lane & 7) ^ (row & 7)) << 4));
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = t[q];
                if (RES) {
                    x3_wait_younger(mt);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        asm volatile("" : "+v"(r[mt & 3][q]));           // from here on the compiler may read the loaded registers
                        v[q] += r[mt & 3][q];
                    }
                }
                MNX_X3_ST(v, mt);
                if (RES && mt + 4 < 8) MNX_X3_LD(r[mt & 3], mt + 4);
            }
#undef MNX_X3_LD
#undef MNX_X3_ST
#undef MNX_X3_LD1
#undef MNX_X3_ST1
            return;
        }
        // ---- 16-bit output: 16-row slabs through the wave's own staging patch, hi plane then (LO_OUT) lo plane ----
        T* crow = C + (size_t)(m0 + wr * 128 + (lane >> 3)) * N + n0 + wc * 64 + (lane & 7) * 8;
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
            v4 lo[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                f32x4 v = acc[mt][nt] * sp.oscale + b4[nt];
                if (EPI == EPI_GELU_16) v = gelu_split4(v);
                v4 hi;
                split16x4<T>(v, hi, lo[nt]);        // (LO_OUT false: the lo half is dead code; hi is derived the same way)
                acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
                *(v4*)(stg + fr * 128 + (((nt * 2 + (fg >> 1)) ^ (fr & 7)) << 4) + (fg & 1) * 8) = hi;
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int row = (lane >> 3) + 8 * i;
                const v8 o8 = *(const v8*)(stg + row * 128 + (((lane & 7) ^ (row & 7)) << 4));
                *(v8*)(crow + (size_t)(mt * 16 + 8 * i) * N) = o8;
            }
            if (LO_OUT) {
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
                    *(v4*)(stg + fr * 128 + (((nt * 2 + (fg >> 1)) ^ (fr & 7)) << 4) + (fg & 1) * 8) = lo[nt];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int row = (lane >> 3) + 8 * i;
                    const v8 o8 = *(const v8*)(stg + row * 128 + (((lane & 7) ^ (row & 7)) << 4));
                    *(v8*)(crow + sp.c_lo + (size_t)(mt * 16 + 8 * i) * N) = o8;
                }
            }
        }
    };
    // counted wait of one phase. `normal` = younger fill instructions at this point of a steady K-tile; in the FIRST K-tile
    // of an output tile (not the stream's first) the epilogue's PST stores and / or the bias DMA (X3_BIAS) are younger too.
    // drain: first / last K-tile of the stream.
#define MNX_X3_WAIT(normal, extra_first)                                         \
    do {                                                                          \
        if (drain) wait_vm<0>();                                                  \
        else if (first_kt) wait_vm<((normal) + (extra_first) > 63 ? 63 : (normal) + (extra_first))>();   /* vmcnt is 6 bits */ \
        else wait_vm<(normal)>();                                                 \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                        \
        __builtin_amdgcn_s_barrier();                                             \
    } while (0)

    int kt = 0, seq = 0;
    for (int g = 0; g < total_kt; ++g) {
        const bool last_kt = (kt == nk - 1);
        const bool has_next = g + 1 < total_kt;
        const bool first_kt = (kt == 0 && seq > 0);
        const bool drain = (g == 0) || !has_next;
        if constexpr (TERMS == 3) {
            // ---- P1: Ah0 . Wl -> rows 0..63.   refill: A lo rows 64-127 of THIS K-tile (its slot was read last in P6)
            fill_a(cur.a + a_lo_b, 1, S_AL1);
            if (first_kt) load_bias(n0);
            read_a(R_AH0{}); read_w(R_WL{});
            // Ah1 (issued in P3 of the previous K-tile). Younger: P4 4, P5 2, P6 2 [, PST stores], this phase's 2 [+ bias]
            MNX_X3_WAIT(10, PST + X3_BIAS);
            mfma_block(MB0{});
            __builtin_amdgcn_s_barrier();
            // ---- P2: Ah1 . Wl -> rows 64..127.   refill: W lo of the next K-tile
            if (has_next) fill_w(nxt.w + w_lo_b, S_WL0);
            read_a(R_AH1{});
            // W hi (issued in P4 of the previous K-tile). Younger: P5 2, P6 2 [, PST stores], P1 2 [+ bias], P2 4
            MNX_X3_WAIT(10, PST + X3_BIAS);
            mfma_block(MB4{});
            __builtin_amdgcn_s_barrier();
            // ---- P3: Ah1 . Wh -> rows 64..127.   refill: A hi rows 64-127 of the next K-tile.   P4 re-reads Ah0: landed before P1
            if (has_next) fill_a(nxt.a, 1, S_AH1);
            read_w(R_WH{});
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            mfma_block(MB4{});
            __builtin_amdgcn_s_barrier();
            // ---- P4: Ah0 . Wh -> rows 0..63.   refill: W hi of the next K-tile (its fragments stay in registers until P6)
            if (has_next) fill_w(nxt.w, S_WH0);
            read_a(R_AH0{});
            // Al0 (issued in P6 of the previous K-tile, before its epilogue). Younger: [PST stores,] P1 2 [+ bias], P2 4, P3 2, P4 4
            MNX_X3_WAIT(12, PST + X3_BIAS);
            mfma_block(MB0{});
            __builtin_amdgcn_s_barrier();
            // ---- P5: Al0 . Wh -> rows 0..63.   refill: A hi rows 0-63 of the next K-tile
            if (has_next) fill_a(nxt.a, 0, S_AH0);
            read_a(R_AL0{});
            // Al1 (issued in P1 of this K-tile, before the bias DMA). Younger: [bias,] P2 4, P3 2, P4 4, P5 2
            MNX_X3_WAIT(12, X3_BIAS);
            mfma_block(MB0{});
            __builtin_amdgcn_s_barrier();
            // ---- P6: Al1 . Wh -> rows 64..127.   refill: A lo rows 0-63 of the next K-tile
            if (has_next) fill_a(nxt.a + a_lo_b, 0, S_AL0);
            read_a(R_AL1{});
            // Ah0', Wl' of the next K-tile (issued in P5 / P2). Younger than Ah0': this phase's 2
            MNX_X3_WAIT(2, 0);
            mfma_block(MB4{});
        } else {
            // A hi rows 0-63 of this K-tile: slot 0 (even K-tiles of the stream) or slot 2 (odd); the next K-tile's goes to the other
            const int ah0_cur = (g & 1) ? S_AL0 : S_AH0, ah0_nxt = (g & 1) ? S_AH0 : S_AL0;
            // ---- P1: Ah0 . Wl -> rows 0..63.   refill: A hi rows 0-63 of the NEXT K-tile (its slot was read last in P4 of the previous one)
            if (has_next) fill_a(nxt.a, 0, ah0_nxt);
            if (first_kt) load_bias(n0);
            read_a_at(ah0_cur * SLOT); read_w(R_WL{});
            // Ah1 (issued in P3 of the previous K-tile). Younger: P4 4 [, PST stores], this phase's 2 [+ bias]
            MNX_X3_WAIT(6, PST + X3_BIAS);
            mfma_block(MB0{});
            __builtin_amdgcn_s_barrier();
            // ---- P2: Ah1 . Wl -> rows 64..127.   refill: W lo of the next K-tile
            if (has_next) fill_w(nxt.w + w_lo_b, S_WL0);
            read_a(R_AH1{});
            // W hi (issued in P4 of the previous K-tile). Younger: [PST stores,] P1 2 [+ bias], P2 4
            MNX_X3_WAIT(6, PST + X3_BIAS);
            mfma_block(MB4{});
            __builtin_amdgcn_s_barrier();
            // ---- P3: Ah1 . Wh -> rows 64..127.   refill: A hi rows 64-127 of the next K-tile.   P4 re-reads Ah0: landed before P1
            if (has_next) fill_a(nxt.a, 1, S_AH1);
            read_w(R_WH{});
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            mfma_block(MB4{});
            __builtin_amdgcn_s_barrier();
            // ---- P4: Ah0 . Wh -> rows 0..63.   refill: W hi of the next K-tile
            if (has_next) fill_w(nxt.w, S_WH0);
            read_a_at(ah0_cur * SLOT);
            // Ah0', Wl' of the next K-tile (issued in P1 — before the bias DMA — and P2). Younger than Wl': P3 2, P4 4
            MNX_X3_WAIT(6, 0);
            mfma_block(MB0{});
        }
        // epilogue placement as gemm256_kernel: second wave row before its closing barrier, first row after its own
        if (last_kt && wr == 1) epilogue();
        __builtin_amdgcn_s_barrier();
        if (last_kt && wr == 0) epilogue();
        cur = nxt;
        advance(nxt);
        if (last_kt) {
            kt = 0; ++seq;
            if (seq < my_tiles) tile_origin(seq, m0, n0);
        } else {
            ++kt;
        }
    }
#undef MNX_X3_WAIT
    if (wr == 0) __builtin_amdgcn_s_barrier();    // the first wave row waits for the second one's last segment
    if (blockIdx.x == 0 && tid == 0) {
        atomicAdd(&x3_clk_acc[0], (unsigned long long)__builtin_readcyclecounter() - clk_c0);
        atomicAdd(&x3_clk_acc[1], (unsigned long long)__builtin_amdgcn_s_memrealtime() - clk_r0);
    }
}

}  // namespace

// The 144 KiB dynamic-LDS opt-in is a per-device, per-function attribute: set once per (device, kernel), so that several
// handles on different GPUs of one process all get it (include/molnextr_hip.h allows that). The once-flag is keyed on the
// kernel VALUE (a type key would be shared by every instantiation with the same signature — all four epilogues of
// gemm256x3_kernel — and only the first one launched would ever opt in).
template <auto Kern>
static hipError_t lds_opt_in(int lds_bytes = P_LDS) {
    static unsigned long long done = 0;          // bit d: device d has the attribute (<= 64 devices per process)
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64 && (__atomic_load_n(&done, __ATOMIC_ACQUIRE) >> dev & 1ull)) return hipSuccess;
    e = hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e == hipSuccess && dev >= 0 && dev < 64) __atomic_fetch_or(&done, 1ull << dev, __ATOMIC_RELEASE);
    return e;
}

// gemm256x3_kernel: split dtypes, any of the four epilogues, whole 256x256 tiles, >= 2 K-tiles.
bool gemm256x3_supports(int dtype, int epi, int M, int N, int K) {
    if (!dt_split(dtype)) return false;
    if (epi != EPI_BIAS_16 && epi != EPI_GELU_16 && epi != EPI_RESID_F32 && epi != EPI_BIAS_F32) return false;
    return M > 0 && M % TM == 0 && N % TN == 0 && K % TK == 0 && K >= 2 * TK;
}

// Instantiated forms: three terms with both output planes (every split layer of FP16X3 / BF16X3), and for fp16 the forms
// FP16X3M needs — two terms (any epilogue) and a GELU output that keeps the hi plane only (fc1 when fc2 runs on two terms;
// the bias epilogue — qkv — always feeds the three-term attention: launch_gemm16 refuses it with one plane).
// bf16 operands never run on two terms (a bf16 hi plane alone is the plain bf16 mode).
hipError_t launch_gemm256x3(int dtype, int epi, const void* A, const void* W, void* C, const float* bias,
                            const float* resid, int M, int N, int K, hipStream_t s, const SplitArgs* sp) {
    if (!sp || (sp->terms != 3 && sp->terms != 2) || !gemm256x3_supports(dtype, epi, M, N, K)) return hipErrorInvalidValue;
    if (epi == EPI_RESID_F32 && !resid) return hipErrorInvalidValue;
    if (!bias) return hipErrorInvalidValue;     // callers without a bias pass a zero vector (the engine keeps one)
    const bool out16 = (epi == EPI_BIAS_16 || epi == EPI_GELU_16);
    if (sp->c_planes != 1 && sp->c_planes != 2) return hipErrorInvalidValue;
    const bool lo_out = !out16 || sp->c_planes == 2;
    if (dtype != MNX_DT_F16X3 && (sp->terms != 3 || !lo_out)) return hipErrorInvalidValue;
    const SplitArgs spv = *sp;
    const int tm = M / TM, tn = N / TN;
    const int grid = tm * tn < PERSISTENT_CUS ? tm * tn : PERSISTENT_CUS;
#define MNX_G256X3_GO(TT, E, TERMS, LO)                                                                                    \
    do {                                                                                                                  \
        const hipError_t attr = lds_opt_in<gemm256x3_kernel<TT, E, TERMS, LO>>(X3_LDS);                                     \
        if (attr != hipSuccess) return attr;                                                                              \
        hipLaunchKernelGGL((gemm256x3_kernel<TT, E, TERMS, LO>), dim3(grid), dim3(512), X3_LDS, s, (const TT*)A,          \
                           (const TT*)W, C, bias, resid, M, N, K, tn, tm * tn, spv);                                      \
    } while (0)
    if (dtype == MNX_DT_BF16X3) {
        switch (epi) {
            case EPI_BIAS_16: MNX_G256X3_GO(bf16_t, EPI_BIAS_16, 3, true); break;
            case EPI_GELU_16: MNX_G256X3_GO(bf16_t, EPI_GELU_16, 3, true); break;
            case EPI_RESID_F32: MNX_G256X3_GO(bf16_t, EPI_RESID_F32, 3, true); break;
            default: MNX_G256X3_GO(bf16_t, EPI_BIAS_F32, 3, true); break;
        }
    } else if (spv.terms == 3) {
        switch (epi) {
            case EPI_BIAS_16: MNX_G256X3_GO(f16_t, EPI_BIAS_16, 3, true); break;
            case EPI_GELU_16: if (lo_out) MNX_G256X3_GO(f16_t, EPI_GELU_16, 3, true); else MNX_G256X3_GO(f16_t, EPI_GELU_16, 3, false); break;
            case EPI_RESID_F32: MNX_G256X3_GO(f16_t, EPI_RESID_F32, 3, true); break;
            default: MNX_G256X3_GO(f16_t, EPI_BIAS_F32, 3, true); break;
        }
    } else {
        switch (epi) {
            case EPI_BIAS_16: MNX_G256X3_GO(f16_t, EPI_BIAS_16, 2, true); break;
            case EPI_GELU_16: if (lo_out) MNX_G256X3_GO(f16_t, EPI_GELU_16, 2, true); else MNX_G256X3_GO(f16_t, EPI_GELU_16, 2, false); break;
            case EPI_RESID_F32: MNX_G256X3_GO(f16_t, EPI_RESID_F32, 2, true); break;
            default: MNX_G256X3_GO(f16_t, EPI_BIAS_F32, 2, true); break;
        }
    }
#undef MNX_G256X3_GO
    return hipGetLastError();
}

// shader clock (MHz) averaged over the gemm256x3_kernel launches since the last reset (0 when there were none)
hipError_t x3_clock_read(double* mhz, bool reset) {
    unsigned long long acc[2] = {0, 0};
    hipError_t e = hipMemcpyFromSymbol(acc, HIP_SYMBOL(x3_clk_acc), sizeof(acc));
    if (e != hipSuccess) return e;
    *mhz = acc[1] ? (double)acc[0] / (double)acc[1] * 100.0 : 0.0;
    if (reset) { acc[0] = acc[1] = 0; e = hipMemcpyToSymbol(HIP_SYMBOL(x3_clk_acc), acc, sizeof(acc)); }
    return e;
}

// ---- what the matrix pipes sustain on random operands (tools/probes/mfma_power.hip as a library call): register-only loop of
// v_mfma_f32_16x16x32_f16, 8 accumulators per wave, 8 waves per CU on every CU, operands rotating through four A and four B
// registers of random fp16 numbers; no LDS, no memory. The honest ceiling of any fp16 MFMA kernel on THIS device under THIS
// power budget: 1.93 PFLOP/s at 1.89 GHz where the nominal peak says 2.5 at 2.4 (profiles/r05_mfma_power.txt).
namespace {
__device__ unsigned long long mfma_probe_clk[2];
__global__ __launch_bounds__(512) void mfma_probe_kernel(float* out, int iters) {
    typedef H16<f16_t>::v8 v8;
    v8 a[4], b[4];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 8; ++j) {
            unsigned h = ((threadIdx.x * 8 + i) * 16 + j + blockIdx.x * 65536) * 2654435761u;
            h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
            a[i][j] = (f16_t)(((int)(h & 0xffff) - 32768) * (1.0f / 32768.f));
            b[i][j] = (f16_t)(((int)(h >> 16) - 32768) * (1.0f / 32768.f));
        }
    unsigned long long c0 = 0, r0 = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) { c0 = __builtin_readcyclecounter(); r0 = __builtin_amdgcn_s_memrealtime(); }
    f32x4 acc[8];
    for (int i = 0; i < 8; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = H16<f16_t>::mfma(a[i & 3], b[(i >> 1) & 3], acc[i]);
    }
    float sum = 0.f;
    for (int i = 0; i < 8; ++i) sum += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        mfma_probe_clk[0] = (unsigned long long)__builtin_readcyclecounter() - c0;
        mfma_probe_clk[1] = (unsigned long long)__builtin_amdgcn_s_memrealtime() - r0;
    }
    if (sum == 12345.678f) out[0] = sum;      // never true: keeps the loop alive
}
}  // namespace

hipError_t mfma_probe(int iters, hipStream_t s, double* tflops, double* mhz) {
    float* scratch = nullptr;        // the kernel's never-taken store needs an address of its own (measurement path: not timed)
    hipError_t e = hipMalloc((void**)&scratch, sizeof(float));
    if (e != hipSuccess) return e;
    hipEvent_t e0, e1;
    e = hipEventCreate(&e0);
    if (e != hipSuccess) { (void)hipFree(scratch); return e; }
    if ((e = hipEventCreate(&e1)) != hipSuccess) { (void)hipEventDestroy(e0); (void)hipFree(scratch); return e; }
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(256), dim3(512), 0, s, scratch, iters / 8 + 1);    // power management settles
    e = hipEventRecord(e0, s);
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(256), dim3(512), 0, s, scratch, iters);
    if (e == hipSuccess) e = hipEventRecord(e1, s);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    unsigned long long clk[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyFromSymbol(clk, HIP_SYMBOL(mfma_probe_clk), sizeof(clk));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(scratch);
    if (e != hipSuccess) return e;
    *tflops = 256.0 * 8.0 * (double)iters * 8.0 * (16.0 * 16.0 * 32.0 * 2.0) / ((double)ms * 1e-3) * 1e-12;
    *mhz = clk[1] ? (double)clk[0] / (double)clk[1] * 100.0 : 0.0;
    return hipSuccess;
}

bool gemm256_supports(int dtype, int epi, int M, int N, int K) {
    if (dtype != MNX_DT_BF16 && dtype != MNX_DT_F16 && !dt_split(dtype)) return false;
    if (epi != EPI_BIAS_16 && epi != EPI_GELU_16) return false;
    if (M % TM || N % TN || K % TK || K < 2 * TK) return false;
    // one workgroup per CU walks tiles in rounds of 256: below one round, or when the last round is mostly empty, the
    // 128x128 kernel fills the chip better
    const int tiles = (M / TM) * (N / TN), rounds = (tiles + 255) / 256;
    return tiles >= 256 && tiles * 10 >= rounds * 256 * 7;
}

hipError_t launch_gemm256(int dtype, int epi, const void* A, const void* W, void* C, const float* bias, int M, int N,
                          int K, hipStream_t s, const SplitArgs* sp) {
    if (!bias || M % TM || N % TN || K % TK || K < 2 * TK) return hipErrorInvalidValue;
    const bool split = dt_split(dtype);
    if (split && (!sp || sp->terms < 1 || sp->terms > 3)) return hipErrorInvalidValue;
    const SplitArgs spv = split ? *sp : SplitArgs();
    if (split && spv.terms >= 2)        // three / two terms: the shared-fill six- / four-phase kernel
        return launch_gemm256x3(dtype, epi, A, W, C, bias, nullptr, M, N, K, s, sp);
    // one term: gemm256_kernel<SPLIT> stores hi AND lo (its counted waits assume both planes' stores); with c_planes == 1 it
    // would write the lo plane c_lo = 0 elements behind the hi plane, over it
    if (split && spv.c_planes != 2) return hipErrorInvalidValue;
    const int tm = M / TM, tn = N / TN;
    const int grid = tm * tn < 256 ? tm * tn : 256;
#define MNX_G256_CASE(TT, E, SP)                                                                                          \
    case E: {                                                                                                             \
        const hipError_t attr = lds_opt_in<gemm256_kernel<TT, E, SP>>();                                                    \
        if (attr != hipSuccess) return attr;                                                                              \
        hipLaunchKernelGGL((gemm256_kernel<TT, E, SP>), dim3(grid), dim3(512), P_LDS, s, (const TT*)A, (const TT*)W,      \
                           (TT*)C, bias, M, N, K, tn, tm * tn, spv);                                                      \
        break;                                                                                                            \
    }
#define MNX_G256_TYPE(TT, SP)                                                                                             \
    switch (epi) { MNX_G256_CASE(TT, EPI_BIAS_16, SP) MNX_G256_CASE(TT, EPI_GELU_16, SP) default: return hipErrorInvalidValue; }
    if (dtype == MNX_DT_F16) { MNX_G256_TYPE(f16_t, false) }
    else if (dtype == MNX_DT_BF16) { MNX_G256_TYPE(bf16_t, false) }
    else if (dtype == MNX_DT_F16X3) { MNX_G256_TYPE(f16_t, true) }
    else if (dtype == MNX_DT_BF16X3) { MNX_G256_TYPE(bf16_t, true) }
    else return hipErrorInvalidValue;
#undef MNX_G256_TYPE
#undef MNX_G256_CASE
    return hipGetLastError();
}

}  // namespace mnx

