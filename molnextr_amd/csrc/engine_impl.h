// engine_impl.h — what the three host files of libmolnextr_hip.so share (internal): the engine behind an mnx_engine handle, the
// two error macros, and the few internals of engine.hip that engine_lab.hip calls too. engine.hip is the model path,
// engine_tables.hip the entry points of the packed-table layer, engine_lab.hip the test aids and probes.
#pragma once
#include "../../include/molnextr_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "dec_types.h"
#include "table_types.h"

namespace mnx {

// One GEMM weight in its operand form: a single 16-bit (or fp32) plane, or — split modes — a hi plane with the lo plane
// `lo` elements behind it, both holding 2^k * W (k per matrix, fp16 split only); oscale = 2^-k.
struct W16 {
    void* p = nullptr;
    size_t lo = 0;
    float oscale = 1.f;
};
struct BlockW {
    float *ln1_g, *ln1_b, *table, *qkv_b, *proj_b, *ln2_g, *ln2_b, *fc1_b, *fc2_b;
    W16 qkv_w, proj_w, fc1_w, fc2_w;
};
struct StageW {
    std::vector<BlockW> blocks;
    float *m_g = nullptr, *m_b = nullptr;
    W16 m_w;
    int C = 0, heads = 0;
};
// op classes of the split modes (mnx_set_split_terms)
enum { SPL_QKV = 1, SPL_ATTN = 2, SPL_PROJ = 4, SPL_FC1 = 8, SPL_FC2 = 16, SPL_MERGE = 32, SPL_ALL = 63 };
struct GraphKey {
    int slots, rows, trace, forced, tile, guided;
    bool operator<(const GraphKey& o) const {
        return std::tie(slots, rows, trace, forced, tile, guided) < std::tie(o.slots, o.rows, o.trace, o.forced, o.tile, o.guided);
    }
};

}  // namespace mnx

struct mnx_engine {
    mnx_config cfg;
    int device = 0;
    std::string err;
    std::vector<void*> allocs;
    size_t bytes = 0;
    // encoder
    float *pe_wt = nullptr, *pe_b = nullptr, *pe_g = nullptr, *pe_beta = nullptr, *fn_g = nullptr, *fn_b = nullptr;
    std::vector<mnx::StageW> stages;
    float *xa = nullptr, *xb = nullptr;              // fp32 residual stream ping-pong
    void *xn16 = nullptr, *qkv16 = nullptr, *attn16 = nullptr, *h16 = nullptr;
    size_t xn_lo = 0, qkv_lo = 0, attn_lo = 0, h_lo = 0;   // split modes: element offset of each buffer's lo plane
    int dt = 0;                                             // kernels.h MNX_DT_* the encoder kernels run (FP16X3M -> MNX_DT_F16X3)
    int split_mask = mnx::SPL_ALL;                          // op classes evaluated with their full term count (others: hi.hi only)
    // per stage: op classes whose full term count is TWO (ah.wh + ah.wl) in the blocks [two_first, two_last] of the stage (the
    // patch-merging reduction counts as the stage's last block): FP16X3M, mnx_set_op_terms
    int two_mask[4] = {0, 0, 0, 0};
    int two_first[4] = {0, 0, 0, 0}, two_last[4] = {1 << 30, 1 << 30, 1 << 30, 1 << 30};
    int* enc_flag = nullptr;                                // device: set when the final LayerNorm sees a non-finite row
    float* zero_bias = nullptr;                             // [2 * widest C] zeros: the bias of the patch-merging reductions
    int zero_bias_n = 0;
    int tap_item = -1;
    float* tap_dst = nullptr;
    // decoder
    mnx::DecWeights dw{};
    mnx::DecBuffers db{};
    float* out_trace = nullptr;
    int* forced_ids = nullptr;  // [32, max_len] teacher-forcing ids of mnx_decode_forced (lazy; test aid)
    int* script_nact = nullptr; // [max_len] n_active of every step of mnx_beam_scripted (lazy; test aid)
    int* beam_script = nullptr; // [2][max_len][32 x 8] parents, then ids, of mnx_decode_beam_forced (lazy; test aid)
    int* lin_script = nullptr;  // [MAX_SLOTS][4] scripted rows {slot, t, prev_tok, rowc} of mnx_dec_linear (lazy; test aid)
    int* guide_labels = nullptr;   // [dec_slots, max_len + 2] label row of every slot, {ids held, the ids}: label-guided decoding
                                   // (mnx_decode_guided / mnx_predict_guided; lazy, written at admission — dec_types.h GuideRows)
    mnx::BeamBuffers beam{};        // allocated lazily on the first mnx_decode_beam
    int* prep_bbox = nullptr;  // scratch of mnx_preprocess
    int* prep_bbox_batch = nullptr;   // [MNX_PREP_MAX_PAGES][4]: scratch of mnx_preprocess_batch (its own: the two may not share)
    float* beam_hidden = nullptr;   // mnx_predict_beam: [32, max_len, dec_dim] decoder outputs of the winners (lazy)
    int* host_flag = nullptr;  // pinned: [2][1 + MAX_CHUNKS] poll snapshots + slot lists
    std::map<mnx::GraphKey, hipGraphExec_t> graphs;
    // continuous-batching pipeline (mnx_predict)
    hipStream_t enc_stream = nullptr;
    float* feat_ring[2] = {nullptr, nullptr};
    hipEvent_t ev_enc_done[2] = {nullptr, nullptr}, ev_feat_free[2] = {nullptr, nullptr}, ev_poll[2] = {nullptr, nullptr};
    int* slot_lists = nullptr;          // device [MAX_CHUNKS][32]: slot list of every 32-slot row tile
    int* rowc_seq = nullptr;            // device [MAX_REF_BATCH]: 0, 1, 2, ... (row indices of a chunk's tiles at admission)
    mnx::TokenClasses* tc_dev = nullptr;
    bool have_tc = false;
    mnx::VocabText* vt_dev = nullptr;        // names of the symbol ids (mnx_set_vocab_text), read by mnx_graph_pack
    bool have_vt = false;
    mnx::SymbolTables* st_dev = nullptr;     // R-group and abbreviation names (mnx_set_symbol_tables), read by mnx_molfile_pack and mnx_smiles_pack
    bool have_st = false;
    int st_n = 0;                       // names of the last mnx_set_symbol_tables
    unsigned char st_kind[512] = {};    // ... and their kinds, which mnx_set_fragments tests frag_of_name against
    void* frag_dev = nullptr;           // the fragment library (mnx_set_fragments): one allocation, fv points into it; read by mnx_expand_pack
    mnx::FragView fv{};
    bool have_frag = false;
    int n_chunk_bufs = 0;
    bool use_graph = true;
    // greedy ticks of up to dec_fused_max rows run as three launches per layer (dec_fused.hip): dec_tile rows per workgroup in
    // the two attention stages (256 threads per row), dec_tile_ff rows in the feed-forward stage; larger ticks keep the
    // 8-launches-per-layer kernels of decoder.hip (knobs MNX_DEC_TILE, MNX_DEC_TILE_FF, MNX_DEC_FUSED_MAX);
    // dec_tile -1: 2 rows per workgroup up to 64 rows of capacity, 4 beyond
    int dec_tile = -1, dec_tile_ff = 4, dec_fused_max = 128;
    // ticks of more than dec_fused_max and up to dec_mid_max rows run the MID form (dec_fused.hip: dec_fa cut into a 16-row
    // linear launch and an attention launch, 4 launches per layer; bit-identical to the fused form, so that the capacity the
    // host happens to pick — it follows poll timing — is invisible in the results up to dec_mid_max rows); beyond that the
    // 8-launches-per-layer kernels of decoder.hip, whose 32-row linears move the fewest bytes per row (MNX_DEC_MID_MAX;
    // 4096 = every capacity: bit-reproducible jobs of any size, slower at >= 1024 rows)
    int dec_mid_max = 0;
    hipStream_t own_stream = nullptr;   // used when the caller passes the legacy null stream (not capturable)
    // profiling (bench aid)
    bool profiling = false;
    int prof_stride = 1;       // bracket the GEMMs of every prof_stride-th mnx_encode call ...
    int prof_calls = 0;        // ... counted since mnx_profile_enable
    int prof_groups = 0;       // encode calls bracketed so far (capped: the event pool stays small)
    int prof_max_groups = 4;
    struct Ev { hipEvent_t a, b; double work; int kind; };   // kind 0 / 4 GEMM (work = FLOP; 4 = block Linears with C >= 512), 1 LayerNorm, 2 window attention, 3 patch embed (work = algorithmic HBM bytes)
    std::vector<Ev> ev_pool;
    size_t ev_used = 0;
};

#define HIPCHK(h, expr)                                                                                   \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) {                                                                           \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                                 \
            return MNX_ERR_HIP;                                                                           \
        }                                                                                                 \
    } while (0)

#define MNXCHK(expr)                                                                                      \
    do {                                                                                                  \
        const int rc_ = (expr);                                                                           \
        if (rc_ != MNX_OK) return rc_;                                                                    \
    } while (0)

namespace mnx {

// engine.hip: selects the engine's device; *s = the caller's stream, or the engine's own for the legacy null stream
int caller_stream(mnx_engine* h, void* stream, hipStream_t* s);

// A device buffer allocated by the first call that needs it and kept (allocs, bytes) until mnx_destroy
template <typename T>
int lazy_alloc(mnx_engine* h, T** p, size_t bytes) {
    if (*p) return MNX_OK;
    HIPCHK(h, hipMalloc((void**)p, bytes));
    h->allocs.push_back(*p);
    h->bytes += bytes;
    return MNX_OK;
}

// Captures what enqueue() puts on s into a graph and instantiates it; the hipGraph_t is released on every path
template <typename F>
int capture_graph(mnx_engine* h, const char* what, hipStream_t s, F&& enqueue, hipGraphExec_t* out) {
    *out = nullptr;
    HIPCHK(h, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    hipGraph_t g = nullptr;
    hipError_t e = enqueue();
    const hipError_t e2 = hipStreamEndCapture(s, &g);
    if (e == hipSuccess) e = e2;
    const char* step = "capture";
    if (e == hipSuccess) {
        step = "instantiate";
        e = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
    }
    if (g) hipGraphDestroy(g);
    if (e != hipSuccess) {
        *out = nullptr;
        h->err = std::string(what) + " " + step + " failed: " + hipGetErrorString(e);
        return MNX_ERR_HIP;
    }
    return MNX_OK;
}

// The step loop of mnx_decode_greedy / beam search: up to max_len steps in groups of 8 (a replay of exec each, or — no
// graph — enqueue()); after every group the begin kernel over `slots` slots counts the alive rows, the host reads the count
// back and stops at 0
template <typename F>
int run_steps(mnx_engine* h, hipGraphExec_t exec, F&& enqueue, int slots, int max_len, hipStream_t s) {
    for (int t = 0; t < max_len; t += 8) {
        for (int i = 0; i < std::min(8, max_len - t); ++i) HIPCHK(h, exec ? hipGraphLaunch(exec, s) : enqueue());
        HIPCHK(h, dec_enqueue_status(h->db, slots, s));
        HIPCHK(h, hipMemcpyAsync(h->host_flag, &h->db.st->n_active, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        if (*h->host_flag == 0) break;
    }
    return MNX_OK;
}

// kept hypotheses of all images (32 images x 8 ... 256 x 1) and how many of them one of B images may keep
constexpr int BEAM_POOL = ROW_TILE * MAX_BEAM;
inline int beam_pool_stride(int B) { return std::min(MAX_BEAM, BEAM_POOL / B); }

// engine.hip: the engine's beam-search buffers set up for B images x `beam` hypotheses; beam search over G reference batches in one
// step sequence (script, logits_trace: mnx_decode_beam_forced alone)
int beam_buffers(mnx_engine* h, int B, int ref_batch, int beam, int n_best, bool hidden);
int decode_beam_groups(mnx_engine* h, const float* const* feats, int G, int ref_batch, int n_total, int beam, int n_best,
                       int max_len, int32_t* tokens, int32_t* lengths, float* scores, float* hidden, hipStream_t s,
                       const int* script = nullptr, float* logits_trace = nullptr);

}  // namespace mnx
