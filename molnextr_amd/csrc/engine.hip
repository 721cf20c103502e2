// engine.hip — host side of libmolnextr_hip.so: weight packing, workspace, encode/decode/edges orchestration,
// hipGraph replay of the decode step. Implements include/molnextr_hip.h.
#include "../../include/molnextr_hip.h"

#include <hip/hip_runtime.h>

#include <time.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "dec_types.h"
#include "kernels.h"
#include "kvq.h"

using namespace mnx;

namespace {

thread_local std::string g_create_error;   // message of the calling thread's last failed mnx_create

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

}  // namespace

#ifndef MNX_PLANE_SKEW
#define MNX_PLANE_SKEW 4352
#endif
static constexpr size_t PLANE_SKEW = MNX_PLANE_SKEW;   // elements (8704 bytes; 16-byte aligned for the LDS-DMA)

struct mnx_engine {
    mnx_config cfg;
    int device = 0;
    std::string err;
    std::vector<void*> allocs;
    size_t bytes = 0;
    // encoder
    float *pe_wt = nullptr, *pe_b = nullptr, *pe_g = nullptr, *pe_beta = nullptr, *fn_g = nullptr, *fn_b = nullptr;
    std::vector<StageW> stages;
    float *xa = nullptr, *xb = nullptr;              // fp32 residual stream ping-pong
    void *xn16 = nullptr, *qkv16 = nullptr, *attn16 = nullptr, *h16 = nullptr;
    size_t xn_lo = 0, qkv_lo = 0, attn_lo = 0, h_lo = 0;   // split modes: element offset of each buffer's lo plane
    int dt = 0;                                             // kernels.h MNX_DT_* the encoder kernels run (FP16X3M -> MNX_DT_F16X3)
    int split_mask = SPL_ALL;                               // op classes evaluated with their full term count (others: hi.hi only)
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
    DecWeights dw{};
    DecBuffers db{};
    float* out_trace = nullptr;
    int* forced_ids = nullptr;  // [32, max_len] teacher-forcing ids of mnx_decode_forced (lazy; test aid)
    int* script_nact = nullptr; // [max_len] n_active of every step of mnx_beam_scripted (lazy; test aid)
    int* beam_script = nullptr; // [2][max_len][32 x 8] parents, then ids, of mnx_decode_beam_forced (lazy; test aid)
    int* guide_labels = nullptr;   // [dec_slots, max_len + 2] label row of every slot, {ids held, the ids}: label-guided decoding
                                   // (mnx_decode_guided / mnx_predict_guided; lazy, written at admission — dec_types.h GuideRows)
    BeamBuffers beam{};        // allocated lazily on the first mnx_decode_beam
    int* prep_bbox = nullptr;  // scratch of mnx_preprocess
    int* prep_bbox_batch = nullptr;   // [MNX_PREP_MAX_PAGES][4]: scratch of mnx_preprocess_batch (its own: the two may not share)
    float* beam_hidden = nullptr;   // mnx_predict_beam: [32, max_len, dec_dim] decoder outputs of the winners (lazy)
    int* host_flag = nullptr;  // pinned: [2][1 + MAX_CHUNKS] poll snapshots + slot lists
    std::map<GraphKey, hipGraphExec_t> graphs;
    // continuous-batching pipeline (mnx_predict)
    hipStream_t enc_stream = nullptr;
    float* feat_ring[2] = {nullptr, nullptr};
    hipEvent_t ev_enc_done[2] = {nullptr, nullptr}, ev_feat_free[2] = {nullptr, nullptr}, ev_poll[2] = {nullptr, nullptr};
    int* slot_lists = nullptr;          // device [MAX_CHUNKS][32]: slot list of every 32-slot row tile
    int* rowc_seq = nullptr;            // device [MAX_REF_BATCH]: 0, 1, 2, ... (row indices of a chunk's tiles at admission)
    TokenClasses* tc_dev = nullptr;
    bool have_tc = false;
    VocabText* vt_dev = nullptr;        // names of the symbol ids (mnx_set_vocab_text), read by mnx_graph_pack
    bool have_vt = false;
    SymbolTables* st_dev = nullptr;     // R-group and abbreviation names (mnx_set_symbol_tables), read by mnx_molfile_pack and mnx_smiles_pack
    bool have_st = false;
    int st_n = 0;                       // names of the last mnx_set_symbol_tables
    void* frag_dev = nullptr;           // the fragment library (mnx_set_fragments): one allocation, fv points into it; read by mnx_expand_pack
    FragView fv{};
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

namespace {

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

struct Packer {
    mnx_engine* h;
    std::unordered_map<std::string, const mnx_weight_desc*> by_name;
    std::vector<std::string> problems;
    float* staging = nullptr;
    size_t staging_elems = 0;

    const mnx_weight_desc* find(const std::string& name, std::initializer_list<int64_t> shape) {
        auto it = by_name.find(name);
        if (it == by_name.end()) {
            problems.push_back("missing " + name);
            return nullptr;
        }
        const mnx_weight_desc* d = it->second;
        bool ok = d->ndim == (int)shape.size() && d->data != nullptr;
        int i = 0;
        for (int64_t s : shape) ok = ok && d->shape[i++] == s;
        if (!ok) {
            std::string got = "[";
            for (int k = 0; k < d->ndim; ++k) got += std::to_string(d->shape[k]) + (k + 1 < d->ndim ? "," : "");
            problems.push_back("shape " + name + ": got " + got + "]");
            return nullptr;
        }
        return d;
    }
    void* dalloc(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) {
            problems.push_back("hipMalloc failed for " + std::to_string(bytes) + " bytes");
            return nullptr;
        }
        h->allocs.push_back(p);
        h->bytes += bytes;
        return p;
    }
    float* up32(const float* host, size_t n) {
        float* p = (float*)dalloc(n * sizeof(float));
        if (p && hipMemcpy(p, host, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            problems.push_back("hipMemcpy H2D failed");
        return p;
    }
    float* f32(const std::string& name, std::initializer_list<int64_t> shape) {
        const mnx_weight_desc* d = find(name, shape);
        if (!d) return nullptr;
        size_t n = 1;
        for (int64_t s : shape) n *= (size_t)s;
        return up32(d->data, n);
    }
    W16 w16(const std::string& name, std::initializer_list<int64_t> shape) {
        W16 w;
        const mnx_weight_desc* d = find(name, shape);
        if (!d) return w;
        size_t n = 1;
        for (int64_t s : shape) n *= (size_t)s;
        if (n > staging_elems) {
            problems.push_back("staging too small for " + name);
            return w;
        }
        const int dt = h->dt;
        float scale = 1.f;
        if (dt == MNX_DT_F16X3) {
            // fp16 split: store 2^k W with max |2^k W| in [2^14, 2^15) — the lo plane of a weight of typical size
            // (|w| ~ 0.02) would be subnormal otherwise; the GEMM epilogue multiplies by 2^-k (exact)
            float mx = 0.f;
            for (size_t i = 0; i < n; ++i) mx = std::max(mx, std::fabs(d->data[i]));
            if (mx > 0.f && std::isfinite(mx)) {
                int e = 0;
                std::frexp(mx, &e);                        // mx = f * 2^e, f in [0.5, 1)
                const int k = std::min(60, std::max(-60, 15 - e));
                scale = std::ldexp(1.f, k);
            }
        }
        w.p = dalloc(n * dt_size(dt));
        if (!w.p) return w;
        w.lo = dt_split(dt) ? n : 0;
        w.oscale = 1.f / scale;
        if (hipMemcpy(staging, d->data, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
            launch_cast16(dt, staging, w.p, n, 0, w.lo, scale) != hipSuccess ||
            hipStreamSynchronize(0) != hipSuccess)
            problems.push_back("convert failed for " + name);
        return w;
    }
    const float* host(const std::string& name, std::initializer_list<int64_t> shape) {
        const mnx_weight_desc* d = find(name, shape);
        return d ? d->data : nullptr;
    }
};

int check_cfg(const mnx_config& c, std::string& why) {
    auto bad = [&](const char* m) { why = m; return MNX_ERR_INVALID_ARG; };
    if (c.n_stages < 1 || c.n_stages > 4) return bad("n_stages must be 1..4");
    if (c.patch != 4) return bad("patch must be 4");
    if (c.window != 12) return bad("window must be 12");
    if (c.embed_dim % 32 || c.embed_dim > 128) return bad("embed_dim must be 32..128, multiple of 32");
    int g = c.img_size / c.patch;
    if (c.img_size % c.patch) return bad("img_size not a multiple of patch");
    for (int s = 0; s < c.n_stages; ++s) {
        int C = c.embed_dim << s;
        if (c.heads[s] * 32 != C) return bad("head_dim must be 32 in every stage");
        if (g % c.window) return bad("every stage's token grid must be a multiple of the window (no padding path)");
        if (c.depths[s] < 1) return bad("depth < 1");
        if (s + 1 < c.n_stages) {
            if (g & 1) return bad("odd grid before merge");
            g /= 2;
        }
    }
    // g x g is the memory the decoder attends over: dec_attn_kernel scores two keys per thread (<= 512), the fused ticks hold
    // PS_CROSS = 160 (tick_tile falls back to the eight-launch tick above that); the reference's 384 x 384 gives 144
    if (g * g > 512) return bad("the encoder's last grid must have <= 512 positions (the cross-attention kernels hold 512 keys)");
    if (c.dec_dim != 256 || c.dec_heads != 8) return bad("decoder kernels are built for d_model 256, 8 heads");
    if (c.dec_layers < 1 || c.dec_layers > MAX_DEC_LAYERS) return bad("dec_layers out of range");
    if (c.dec_ff % 256 || c.dec_ff < 256) return bad("dec_ff must be a multiple of 256");
    if (c.vocab > 256 || c.vocab != c.sym_offset + 2 * c.coord_bins) return bad("vocab must be sym_offset+2*bins <= 256");
    if (c.max_len < 1 || c.max_len > 512) return bad("max_len must be 1..512");
    if (c.max_batch < 1) return bad("max_batch < 1");
    if (c.max_atoms < 1 || c.max_atoms > 256) return bad("max_atoms must be 1..256");
    if (c.compute_dtype < MNX_DTYPE_BF16 || c.compute_dtype > MNX_DTYPE_FP16X3M) return bad("compute_dtype");
    if (c.dec_slots < 0 || c.dec_slots > MAX_SLOTS || (c.dec_slots % ROW_TILE) != 0) return bad("dec_slots");
    if (c.pe_len < ROW_TILE) return bad("pe_len too small");
    return MNX_OK;
}

// the compute_dtype's own two-term table on encoder stage st: none, or for FP16X3M the header's
// MNX_FP16X3M_TWO_TERM_BY_STAGE / _FIRST_BLOCK_BY_STAGE, written for Swin-B's four stages — a shallower encoder (the tests'
// tiny one) keeps its LAST stages' rows
void install_mode_terms(mnx_engine* h, int st) {
    const int by_stage[4] = MNX_FP16X3M_TWO_TERM_BY_STAGE, first[4] = MNX_FP16X3M_FIRST_BLOCK_BY_STAGE;
    const bool m = h->cfg.compute_dtype == MNX_DTYPE_FP16X3M;
    const int row = st + 4 - h->cfg.n_stages;
    h->two_mask[st] = m ? by_stage[row] : 0;
    h->two_first[st] = m ? first[row] : 0;
    h->two_last[st] = 1 << 30;
}

}  // namespace

extern "C" {

int mnx_abi_version(void) { return MNX_ABI_VERSION; }

const char* mnx_last_error(const mnx_engine* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

size_t mnx_workspace_bytes(const mnx_engine* h) { return h ? h->bytes : 0; }

void mnx_destroy(mnx_engine* h) {
    if (!h) return;
    hipSetDevice(h->device);
    if (const char* sp = getenv("MNX_FUSED_STAMPS")) { (void)hipDeviceSynchronize(); dec_fused_dump_stamps(sp); }   // lab aid
    for (auto& kv : h->graphs) hipGraphExecDestroy(kv.second);
    if (h->own_stream) hipStreamDestroy(h->own_stream);
    if (h->enc_stream) hipStreamDestroy(h->enc_stream);
    for (int i = 0; i < 2; ++i) {
        if (h->ev_enc_done[i]) hipEventDestroy(h->ev_enc_done[i]);
        if (h->ev_feat_free[i]) hipEventDestroy(h->ev_feat_free[i]);
        if (h->ev_poll[i]) hipEventDestroy(h->ev_poll[i]);
    }
    for (auto& ev : h->ev_pool) { hipEventDestroy(ev.a); hipEventDestroy(ev.b); }
    for (void* p : h->allocs) hipFree(p);
    if (h->frag_dev) hipFree(h->frag_dev);
    if (h->host_flag) hipHostFree(h->host_flag);
    delete h;
}

int mnx_create(const mnx_config* cfg, const mnx_weight_desc* weights, int32_t n_weights, int32_t device,
               mnx_engine** out) {
    if (out) *out = nullptr;
    if (!cfg || !weights || !out || n_weights <= 0) {
        g_create_error = "mnx_create: null argument";
        return MNX_ERR_INVALID_ARG;
    }
    std::string why;
    if (check_cfg(*cfg, why) != MNX_OK) {
        g_create_error = "mnx_create: bad config: " + why;
        return MNX_ERR_INVALID_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        g_create_error = "mnx_create: no HIP device " + std::to_string(device) + " (libmolnextr_hip needs an MI355X; there is no CPU fallback)";
        return MNX_ERR_NO_DEVICE;
    }
    hipDeviceProp_t prop;
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) {
        g_create_error = "mnx_create: cannot select device";
        return MNX_ERR_NO_DEVICE;
    }
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
        g_create_error = std::string("mnx_create: device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
        return MNX_ERR_NO_DEVICE;
    }
    mnx_engine* h = new mnx_engine();
    h->cfg = *cfg;
    h->device = device;
    // FP16X3M = the FP16X3 kernels and weights with the op classes of MNX_FP16X3M_TWO_TERM_BY_STAGE on two product terms
    h->dt = cfg->compute_dtype == MNX_DTYPE_FP16X3M ? MNX_DT_F16X3 : cfg->compute_dtype;
    for (int st = 0; st < cfg->n_stages; ++st) install_mode_terms(h, st);
    const char* ng = getenv("MNX_NO_GRAPH");
    h->use_graph = !(ng && ng[0] == '1');
    if (const char* e = getenv("MNX_DEC_TILE")) h->dec_tile = atoi(e);              // 0: never use the fused tick
    if (const char* e = getenv("MNX_DEC_TILE_FF")) h->dec_tile_ff = atoi(e);
    if (const char* e = getenv("MNX_DEC_FUSED_MAX")) h->dec_fused_max = atoi(e);    // largest capacity that runs fused
    if (const char* e = getenv("MNX_DEC_MID_MAX")) h->dec_mid_max = atoi(e);        // largest capacity that runs the mid form
    // dec_fused.hip instantiates (attention rows, feed-forward rows) = (2, 4) (2, 8) (4, 4) (4, 8) (4, 16): 16-row feed-forward
    // tiles only go with 4-row attention tiles (auto picks 2 rows up to 64 rows of capacity) — refused here, not at the first tick
    if ((h->dec_tile != -1 && h->dec_tile != 0 && h->dec_tile != 2 && h->dec_tile != 4) ||
        (h->dec_tile_ff != 4 && h->dec_tile_ff != 8 && h->dec_tile_ff != 16) ||
        (h->dec_tile_ff == 16 && h->dec_tile != 4 && h->dec_tile != 0)) {
        g_create_error = "mnx_create: MNX_DEC_TILE must be -1 (auto), 0, 2 or 4 and MNX_DEC_TILE_FF 4, 8 or 16 (16 only with MNX_DEC_TILE=4)";
        delete h;
        return MNX_ERR_INVALID_ARG;
    }
    Packer P;
    P.h = h;
    for (int i = 0; i < n_weights; ++i)
        if (weights[i].name) P.by_name[weights[i].name] = &weights[i];
    const mnx_config& c = h->cfg;

    // staging buffer for fp32 -> 16-bit conversion: the largest GEMM weight
    size_t max_w = 0;
    for (int s = 0; s < c.n_stages; ++s) {
        size_t C = (size_t)c.embed_dim << s;
        max_w = std::max(max_w, 4 * C * C);
        if (s + 1 < c.n_stages) max_w = std::max(max_w, 8 * C * C);
    }
    P.staging_elems = max_w;
    if (hipMalloc((void**)&P.staging, max_w * sizeof(float)) != hipSuccess) {
        g_create_error = "mnx_create: hipMalloc(staging) failed";
        delete h;
        return MNX_ERR_HIP;
    }

    // ---------------- encoder weights ----------------
    const std::string T = "transformer.";
    {
        const int C = c.embed_dim;
        const float* pw = P.host(T + "patch_embed.proj.weight", {C, 3, 4, 4});
        if (pw) {  // [C][48] -> [48][C]
            std::vector<float> wt((size_t)48 * C);
            for (int ch = 0; ch < C; ++ch)
                for (int i = 0; i < 48; ++i) wt[(size_t)i * C + ch] = pw[(size_t)ch * 48 + i];
            h->pe_wt = P.up32(wt.data(), wt.size());
        }
        h->pe_b = P.f32(T + "patch_embed.proj.bias", {C});
        h->pe_g = P.f32(T + "patch_embed.norm.weight", {C});
        h->pe_beta = P.f32(T + "patch_embed.norm.bias", {C});
    }
    const int64_t NT = (2 * c.window - 1) * (2 * c.window - 1);
    h->stages.resize(c.n_stages);
    for (int s = 0; s < c.n_stages; ++s) {
        StageW& st = h->stages[s];
        const int64_t C = (int64_t)c.embed_dim << s;
        st.C = (int)C;
        st.heads = c.heads[s];
        for (int b = 0; b < c.depths[s]; ++b) {
            const std::string p = T + "layers." + std::to_string(s) + ".blocks." + std::to_string(b) + ".";
            BlockW w{};
            w.ln1_g = P.f32(p + "norm1.weight", {C});
            w.ln1_b = P.f32(p + "norm1.bias", {C});
            w.table = P.f32(p + "attn.relative_position_bias_table", {NT, st.heads});
            w.qkv_w = P.w16(p + "attn.qkv.weight", {3 * C, C});
            w.qkv_b = P.f32(p + "attn.qkv.bias", {3 * C});
            w.proj_w = P.w16(p + "attn.proj.weight", {C, C});
            w.proj_b = P.f32(p + "attn.proj.bias", {C});
            w.ln2_g = P.f32(p + "norm2.weight", {C});
            w.ln2_b = P.f32(p + "norm2.bias", {C});
            w.fc1_w = P.w16(p + "mlp.fc1.weight", {4 * C, C});
            w.fc1_b = P.f32(p + "mlp.fc1.bias", {4 * C});
            w.fc2_w = P.w16(p + "mlp.fc2.weight", {C, 4 * C});
            w.fc2_b = P.f32(p + "mlp.fc2.bias", {C});
            st.blocks.push_back(w);
        }
        if (s + 1 < c.n_stages) {
            const std::string p = T + "layers." + std::to_string(s) + ".downsample.";
            st.m_g = P.f32(p + "norm.weight", {4 * C});
            st.m_b = P.f32(p + "norm.bias", {4 * C});
            st.m_w = P.w16(p + "reduction.weight", {2 * C, 4 * C});
        }
    }
    const int64_t CF = (int64_t)c.embed_dim << (c.n_stages - 1);
    h->fn_g = P.f32(T + "norm.weight", {CF});
    h->fn_b = P.f32(T + "norm.bias", {CF});

    // ---------------- decoder weights ----------------
    DecWeights& dw = h->dw;
    const int64_t D = c.dec_dim, FF = c.dec_ff, V = c.vocab;
    const int64_t S = (int64_t)(c.img_size / c.patch >> (c.n_stages - 1)) * (c.img_size / c.patch >> (c.n_stages - 1));
    dw.layers = c.dec_layers; dw.heads = c.dec_heads; dw.dff = c.dec_ff; dw.vocab = c.vocab; dw.vpad = (c.vocab + 7) & ~7;
    dw.sym_offset = c.sym_offset; dw.bins = c.coord_bins; dw.pe_len = c.pe_len; dw.enc_dim = (int)CF;
    const std::string Dp = "decoder.chartok_coords.";
    dw.w_enc = P.f32(Dp + "enc_trans_layer.0.weight", {D, CF});
    dw.b_enc = P.f32(Dp + "enc_trans_layer.0.bias", {D});
    dw.lnF_g = P.f32(Dp + "decoder.layer_norm.weight", {D});
    dw.lnF_b = P.f32(Dp + "decoder.layer_norm.bias", {D});
    dw.emb = P.f32(Dp + "embeddings.make_embedding.emb_luts.0.weight", {V, D});
    dw.bout = P.f32(Dp + "output_layer.bias", {V});
    {
        const float* wo = P.host(Dp + "output_layer.weight", {V, D});
        if (wo) {
            std::vector<float> t((size_t)D * dw.vpad, 0.f);
            for (int64_t v = 0; v < V; ++v)
                for (int64_t k = 0; k < D; ++k) t[(size_t)k * dw.vpad + v] = wo[v * D + k];
            dw.wout_t = P.up32(t.data(), t.size());
        }
        // sinusoid table: recomputed exactly as the reference builds it (MolNexTR/models/embedding.py:30-35);
        // if the checkpoint carries pe.pe it must agree.
        std::vector<float> pe((size_t)c.pe_len * D);
        for (int64_t pos = 0; pos < c.pe_len; ++pos)
            for (int64_t i = 0; i < D; i += 2) {
                const float div = expf((float)i * (float)(-(std::log(10000.0) / (double)D)));
                pe[pos * D + i] = sinf((float)pos * div);
                pe[pos * D + i + 1] = cosf((float)pos * div);
            }
        auto it = P.by_name.find(Dp + "embeddings.make_embedding.pe.pe");
        if (it != P.by_name.end() && it->second->data) {
            const mnx_weight_desc* d = it->second;
            if (d->ndim == 3 && d->shape[0] == c.pe_len && d->shape[1] == 1 && d->shape[2] == D)
                memcpy(pe.data(), d->data, pe.size() * sizeof(float));   // take the checkpoint's buffer verbatim
            else
                P.problems.push_back("shape " + Dp + "embeddings.make_embedding.pe.pe");
        }
        dw.pe = P.up32(pe.data(), pe.size());
    }
    // [rows][cols] -> device [cols][rows]: the fused tick reads a weight COLUMN per lane (dec_fused.hip)
    auto upT = [&](const float* src, int64_t rows, int64_t cols) -> const float* {
        if (!src) return nullptr;
        std::vector<float> t((size_t)rows * cols);
        for (int64_t r = 0; r < rows; ++r)
            for (int64_t k = 0; k < cols; ++k) t[(size_t)k * rows + r] = src[(size_t)r * cols + k];
        return P.up32(t.data(), t.size());
    };
    std::vector<float> memkv_w((size_t)c.dec_layers * 2 * D * D), memkv_b((size_t)c.dec_layers * 2 * D);
    bool memkv_ok = true;
    for (int l = 0; l < c.dec_layers; ++l) {
        const std::string p = Dp + "decoder.transformer_layers." + std::to_string(l) + ".";
        DecLayerW& L = dw.L[l];
        L.ln1_g = P.f32(p + "layer_norm_1.weight", {D});
        L.ln1_b = P.f32(p + "layer_norm_1.bias", {D});
        L.ln2_g = P.f32(p + "layer_norm_2.weight", {D});
        L.ln2_b = P.f32(p + "layer_norm_2.bias", {D});
        L.lnf_g = P.f32(p + "feed_forward.layer_norm.weight", {D});
        L.lnf_b = P.f32(p + "feed_forward.layer_norm.bias", {D});
        const float *wq = P.host(p + "self_attn.linear_query.weight", {D, D}), *bq = P.host(p + "self_attn.linear_query.bias", {D});
        const float *wk = P.host(p + "self_attn.linear_keys.weight", {D, D}), *bk = P.host(p + "self_attn.linear_keys.bias", {D});
        const float *wv = P.host(p + "self_attn.linear_values.weight", {D, D}), *bv = P.host(p + "self_attn.linear_values.bias", {D});
        if (wq && wk && wv && bq && bk && bv) {
            std::vector<float> w((size_t)3 * D * D), b((size_t)3 * D);
            memcpy(&w[0], wq, D * D * 4); memcpy(&w[D * D], wk, D * D * 4); memcpy(&w[2 * D * D], wv, D * D * 4);
            memcpy(&b[0], bq, D * 4); memcpy(&b[D], bk, D * 4); memcpy(&b[2 * D], bv, D * 4);
            L.wqkv = P.up32(w.data(), w.size());
            L.bqkv = P.up32(b.data(), b.size());
            L.wqkv_t = upT(w.data(), 3 * D, D);
        }
        L.wo = P.f32(p + "self_attn.final_linear.weight", {D, D});
        L.wo_t = upT(P.host(p + "self_attn.final_linear.weight", {D, D}), D, D);
        L.bo = P.f32(p + "self_attn.final_linear.bias", {D});
        L.wq2 = P.f32(p + "context_attn.linear_query.weight", {D, D});
        L.wq2_t = upT(P.host(p + "context_attn.linear_query.weight", {D, D}), D, D);
        L.bq2 = P.f32(p + "context_attn.linear_query.bias", {D});
        L.wo2 = P.f32(p + "context_attn.final_linear.weight", {D, D});
        L.wo2_t = upT(P.host(p + "context_attn.final_linear.weight", {D, D}), D, D);
        L.bo2 = P.f32(p + "context_attn.final_linear.bias", {D});
        const float *ck = P.host(p + "context_attn.linear_keys.weight", {D, D}), *cbk = P.host(p + "context_attn.linear_keys.bias", {D});
        const float *cv = P.host(p + "context_attn.linear_values.weight", {D, D}), *cbv = P.host(p + "context_attn.linear_values.bias", {D});
        if (ck && cv && cbk && cbv) {
            memcpy(&memkv_w[(size_t)l * 2 * D * D], ck, D * D * 4);
            memcpy(&memkv_w[(size_t)l * 2 * D * D + D * D], cv, D * D * 4);
            memcpy(&memkv_b[(size_t)l * 2 * D], cbk, D * 4);
            memcpy(&memkv_b[(size_t)l * 2 * D + D], cbv, D * 4);
        } else {
            memkv_ok = false;
        }
        L.w1 = P.f32(p + "feed_forward.w_1.weight", {FF, D});
        L.w1_t = upT(P.host(p + "feed_forward.w_1.weight", {FF, D}), FF, D);
        L.b1 = P.f32(p + "feed_forward.w_1.bias", {FF});
        L.w2 = P.f32(p + "feed_forward.w_2.weight", {D, FF});
        L.w2_t = upT(P.host(p + "feed_forward.w_2.weight", {D, FF}), D, FF);
        L.b2 = P.f32(p + "feed_forward.w_2.bias", {D});
    }
    if (memkv_ok) {
        dw.w_memkv = P.up32(memkv_w.data(), memkv_w.size());
        dw.b_memkv = P.up32(memkv_b.data(), memkv_b.size());
    }
    {
        const float *w1 = P.host("decoder.edges.mlp.0.weight", {D, 2 * D}), *b1 = P.host("decoder.edges.mlp.0.bias", {D});
        if (w1 && b1) {
            std::vector<float> w((size_t)2 * D * D), b((size_t)2 * D, 0.f);
            for (int64_t n = 0; n < D; ++n) {
                memcpy(&w[(size_t)n * D], w1 + n * 2 * D, D * 4);              // multiplies h_i
                memcpy(&w[(size_t)(D + n) * D], w1 + n * 2 * D + D, D * 4);    // multiplies h_j
                b[D + n] = b1[n];
            }
            dw.edge_w1cat = P.up32(w.data(), w.size());
            dw.edge_b1cat = P.up32(b.data(), b.size());
        }
        dw.edge_w2 = P.f32("decoder.edges.mlp.2.weight", {7, D});
        dw.edge_b2 = P.f32("decoder.edges.mlp.2.bias", {7});
    }
    hipFree(P.staging);

    // ---------------- workspace ----------------
    const size_t MB = (size_t)c.max_batch;
    const size_t G = c.img_size / c.patch, L0 = G * G, C0 = c.embed_dim;
    size_t max_qkv = 0, max_h = 0, max_xn = 0;
    {
        size_t Ls = L0, Cs = C0;
        for (int s = 0; s < c.n_stages; ++s) {
            max_qkv = std::max(max_qkv, Ls * 3 * Cs);
            max_h = std::max(max_h, Ls * 4 * Cs);
            max_xn = std::max(max_xn, Ls * Cs);
            if (s + 1 < c.n_stages) { Ls /= 4; Cs *= 2; }
        }
    }
    h->xa = (float*)P.dalloc(MB * L0 * C0 * 4);
    h->xb = (float*)P.dalloc(MB * L0 * C0 * 4 / 2);
    // operand bytes per element: 2 (bf16 / fp16), 4 (fp32 parity mode, or the two 16-bit planes of the split modes)
    const size_t es = dt_size(h->dt);
    // split modes: the lo plane follows the hi plane after PLANE_SKEW extra elements, so that the two planes of a row
    // are not a large power of two apart (same HBM channel / bank for every hi / lo pair of a stream)
    const size_t skew = dt_split(h->dt) ? PLANE_SKEW : 0;
    h->xn16 = P.dalloc(MB * max_xn * es + skew * 2);
    h->qkv16 = P.dalloc(MB * max_qkv * es + skew * 2);
    h->attn16 = P.dalloc(MB * max_xn * es + skew * 2);
    h->h16 = P.dalloc(MB * max_h * es + skew * 2);
    if (dt_split(h->dt)) {
        h->xn_lo = MB * max_xn + skew; h->qkv_lo = MB * max_qkv + skew; h->attn_lo = MB * max_xn + skew; h->h_lo = MB * max_h + skew;
    }
    {   // the reference's PatchMerging.reduction has no bias; every GEMM kernel adds this vector instead, so that the rows
        // of a layer that different kernels compute (launch_gemm16 splits by batch size) go through the same additions
        const size_t nz = std::max((size_t)c.embed_dim << c.n_stages, (size_t)4096);   // also the stand-in bias of mnx_gemm16_split
        h->zero_bias = (float*)P.dalloc(nz * sizeof(float));
        h->zero_bias_n = (int)nz;
        if (h->zero_bias && hipMemset(h->zero_bias, 0, nz * sizeof(float)) != hipSuccess) P.problems.push_back("hipMemset failed");
    }
    h->enc_flag = (int*)P.dalloc(sizeof(int));
    if (h->enc_flag && hipMemset(h->enc_flag, 0, sizeof(int)) != hipSuccess) P.problems.push_back("hipMemset failed");
    DecBuffers& db = h->db;
    const int SL = c.dec_slots > 0 ? c.dec_slots : 2048;
    h->n_chunk_bufs = SL / ROW_TILE;   // 32-slot row tiles; a reference batch of n rows holds ceil(n / 32) of them
    db.T = c.max_len; db.S = (int)S; db.slots = SL; db.mem_blocks = h->n_chunk_bufs * ROW_TILE; db.kmax = c.max_atoms;
    db.st = (DecState*)P.dalloc(sizeof(DecState));
    db.x = (float*)P.dalloc((size_t)SL * D * 4);
    db.x2 = (float*)P.dalloc((size_t)SL * D * 4);
    db.part = (float*)P.dalloc((size_t)(FF / 256) * SL * D * 4);
    // partial planes of the fused / mid tick: only ticks of up to max(dec_fused_max, dec_mid_max) rows of capacity touch them
    // (128 rows by default: 4 MB; every slot would be 100 MB at the bench's 3072)
    db.fpart_rows = std::min(SL, std::max(ROW_TILE, (std::max(h->dec_fused_max, h->dec_mid_max) + ROW_TILE - 1) / ROW_TILE * ROW_TILE));
    db.fpart = (float*)P.dalloc((size_t)2 * 16 * db.fpart_rows * D * 4);
    if (db.fpart && hipMemset(db.fpart, 0, (size_t)2 * 16 * db.fpart_rows * D * 4) != hipSuccess) P.problems.push_back("hipMemset failed");
    if (dec_fused_init() != hipSuccess) P.problems.push_back("dec_fused_init: LDS opt-in failed");
    db.q = (float*)P.dalloc((size_t)SL * D * 4);
    db.ctx = (float*)P.dalloc((size_t)SL * D * 4);
    db.h = (float*)P.dalloc((size_t)SL * FF * 4);
    // self K / V and projected memory K / V: 24-bit block fixed point, 100 bytes per cached row of 32 channels (kvq.h)
    db.Tq = kvq_rows(c.max_len); db.Sq = kvq_rows((int)S);
    const size_t cache = (size_t)c.dec_layers * SL * c.dec_heads * kvq_block_bytes(db.Tq);
    db.self_k = (char*)P.dalloc(cache);
    db.self_v = (char*)P.dalloc(cache);
    // every scale of a block must be finite before its first key is written (a lane whose key index is clamped may fetch a row
    // beyond the written ones and multiplies a zero probability by its scale)
    if (db.self_k && db.self_v && (hipMemset(db.self_k, 0, cache) != hipSuccess || hipMemset(db.self_v, 0, cache) != hipSuccess))
        P.problems.push_back("hipMemset failed");
    db.memory = (float*)P.dalloc((size_t)ROW_TILE * S * D * 4);
    db.mem_kv32 = (float*)P.dalloc((size_t)ROW_TILE * S * c.dec_layers * 2 * D * 4);
    const size_t mem_bytes = (size_t)db.mem_blocks * c.dec_layers * 2 * c.dec_heads * kvq_block_bytes(db.Sq);
    db.mem_kv = (char*)P.dalloc(mem_bytes);
    if (db.mem_kv && hipMemset(db.mem_kv, 0, mem_bytes) != hipSuccess) P.problems.push_back("hipMemset failed");
    db.tokens = (int*)P.dalloc((size_t)SL * c.max_len * 4);
    db.logp = (float*)P.dalloc((size_t)SL * c.max_len * 4);
    db.hidden = (float*)P.dalloc((size_t)SL * c.max_len * D * 4);
    db.edge_g = (float*)P.dalloc((size_t)ROW_TILE * db.kmax * D * 4);
    db.edge_uv = (float*)P.dalloc((size_t)ROW_TILE * db.kmax * 2 * D * 4);
    db.edge_prob = (float*)P.dalloc((size_t)ROW_TILE * db.kmax * db.kmax * 8 * 4);
    const size_t ring_rows = std::max<size_t>(ROW_TILE, MB);   // one encode group (max_batch images) per buffer
    h->feat_ring[0] = (float*)P.dalloc(ring_rows * S * CF * 4);
    h->feat_ring[1] = (float*)P.dalloc(ring_rows * S * CF * 4);
    h->slot_lists = (int*)P.dalloc((size_t)MAX_CHUNKS * ROW_TILE * 4);
    h->rowc_seq = (int*)P.dalloc((size_t)MAX_REF_BATCH * 4);
    if (h->rowc_seq) {
        std::vector<int> seq_rows(MAX_REF_BATCH);
        for (int i = 0; i < MAX_REF_BATCH; ++i) seq_rows[i] = i;
        if (hipMemcpy(h->rowc_seq, seq_rows.data(), (size_t)MAX_REF_BATCH * 4, hipMemcpyHostToDevice) != hipSuccess)
            P.problems.push_back("row index table upload failed");
    }
    h->tc_dev = (TokenClasses*)P.dalloc(sizeof(TokenClasses));
    h->vt_dev = (VocabText*)P.dalloc(sizeof(VocabText));
    h->st_dev = (SymbolTables*)P.dalloc(sizeof(SymbolTables));
    h->prep_bbox = (int*)P.dalloc(4 * sizeof(int));   // at create: mnx_preprocess may run beside another entry point
    h->prep_bbox_batch = (int*)P.dalloc((size_t)MNX_PREP_MAX_PAGES * 4 * sizeof(int));
    {
        // Encoder and decoder run concurrently on separate streams; the encoder stream gets the high priority (its
        // large GEMM grids otherwise queue behind the decode ticks' many small kernels: measured +1.6 %). Partitioning
        // the chip with CU masks instead was measured and rejected.
        int lo = 0, hi = 0;
        hipDeviceGetStreamPriorityRange(&lo, &hi);
        if (hipStreamCreateWithPriority(&h->enc_stream, hipStreamNonBlocking, hi) != hipSuccess) P.problems.push_back("stream create failed");
    }
    for (int i = 0; i < 2; ++i)
        if (hipEventCreateWithFlags(&h->ev_enc_done[i], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_feat_free[i], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_poll[i], hipEventDisableTiming) != hipSuccess)
            P.problems.push_back("event create failed");
    if (hipHostMalloc((void**)&h->host_flag, 32768) != hipSuccess) P.problems.push_back("hipHostMalloc failed");

    if (!P.problems.empty()) {
        g_create_error = "mnx_create: " + std::to_string(P.problems.size()) + " problem(s):";
        for (size_t i = 0; i < P.problems.size() && i < 12; ++i) g_create_error += "\n  " + P.problems[i];
        bool weights_bad = false;
        for (auto& p : P.problems) weights_bad = weights_bad || p.rfind("missing", 0) == 0 || p.rfind("shape", 0) == 0;
        mnx_destroy(h);
        return weights_bad ? MNX_ERR_WEIGHTS : MNX_ERR_HIP;
    }
    if (hipDeviceSynchronize() != hipSuccess) {
        g_create_error = "mnx_create: device sync failed";
        mnx_destroy(h);
        return MNX_ERR_HIP;
    }
    *out = h;
    return MNX_OK;
}

int mnx_set_encoder_tap(mnx_engine* h, int32_t item, float* dst) {
    if (!h) return MNX_ERR_INVALID_ARG;
    h->tap_item = item;
    h->tap_dst = dst;
    return MNX_OK;
}

int mnx_set_split_terms(mnx_engine* h, int32_t mask) {
    if (!h) return MNX_ERR_INVALID_ARG;
    if (mask < 0 || mask > SPL_ALL) { h->err = "mnx_set_split_terms: mask must be 0..63"; return MNX_ERR_INVALID_ARG; }
    h->split_mask = mask;
    return MNX_OK;
}

int mnx_set_op_terms(mnx_engine* h, int32_t stage, int32_t two_term_mask, int32_t first_block, int32_t last_block) {
    if (!h) return MNX_ERR_INVALID_ARG;
    if (h->dt != MNX_DT_F16X3) { h->err = "mnx_set_op_terms: compute_dtype must be FP16X3 or FP16X3M"; return MNX_ERR_INVALID_ARG; }
    if (stage < -1 || stage >= h->cfg.n_stages) { h->err = "mnx_set_op_terms: stage must be -1 (all) or 0..n_stages-1"; return MNX_ERR_INVALID_ARG; }
    if (two_term_mask == -1) {      // the mode's own table (first_block / last_block ignored)
        for (int st = 0; st < h->cfg.n_stages; ++st)
            if (stage < 0 || stage == st) install_mode_terms(h, st);
        return MNX_OK;
    }
    if (two_term_mask < 0 || two_term_mask > SPL_ALL || (two_term_mask & SPL_ATTN)) {
        h->err = "mnx_set_op_terms: mask must be -1 (the mode's own table) or a subset of the Linear classes (1 qkv, 4 proj, 8 fc1, 16 fc2, 32 merge)";
        return MNX_ERR_INVALID_ARG;
    }
    if (first_block < 0 || last_block < first_block) { h->err = "mnx_set_op_terms: 0 <= first_block <= last_block required"; return MNX_ERR_INVALID_ARG; }
    for (int st = 0; st < h->cfg.n_stages; ++st)
        if (stage < 0 || stage == st) { h->two_mask[st] = two_term_mask; h->two_first[st] = first_block; h->two_last[st] = last_block; }
    return MNX_OK;
}

int mnx_encoder_status(mnx_engine* h, int32_t* nonfinite, void* stream) {
    if (!h || !nonfinite) return MNX_ERR_INVALID_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    int flag = 0;
    HIPCHK(h, hipMemcpyAsync(&flag, h->enc_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (flag) HIPCHK(h, hipMemsetAsync(h->enc_flag, 0, sizeof(int), s));
    *nonfinite = flag;
    return MNX_OK;
}

// mnx_predict / mnx_predict_beam: after the final synchronisation, turn a non-finite encoder output into an error
static int check_encoder_range(mnx_engine* h, hipStream_t s) {
    int flag = 0;
    HIPCHK(h, hipMemcpyAsync(&flag, h->enc_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (!flag) return MNX_OK;
    HIPCHK(h, hipMemsetAsync(h->enc_flag, 0, sizeof(int), s));
    HIPCHK(h, hipStreamSynchronize(s));
    h->err = "encoder features are not finite (an activation left the fp16 range of compute_dtype FP16 / FP16X3, or the "
             "input holds NaN / Inf): use MNX_DTYPE_BF16X3 or MNX_DTYPE_FP32 for this checkpoint";
    return MNX_ERR_RANGE;
}

// mnx_encode / mnx_encode_gray8: the image source is (pointer, MNX_IMG_* format); only the patch embedding looks at it
static int encode_impl(mnx_engine* h, const char* name, const void* images, int fmt, int32_t B, float* features_out,
                       void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    if (!images || !features_out || B < 1) { h->err = std::string(name) + ": null/empty argument"; return MNX_ERR_INVALID_ARG; }
    if (fmt == MNX_IMG_GRAY8 && ((uintptr_t)images & 3)) { h->err = std::string(name) + ": gray must be 4-byte aligned"; return MNX_ERR_INVALID_ARG; }
    if (B > h->cfg.max_batch) { h->err = std::string(name) + ": B exceeds max_batch"; return MNX_ERR_CAPACITY; }
    hipStream_t s = (hipStream_t)stream;
    const mnx_config& c = h->cfg;
    const int dt = h->dt;
    HIPCHK(h, hipSetDevice(h->device));
    int Hh = c.img_size / c.patch, Ww = Hh, C = c.embed_dim;
    float* cur = h->xa;
    float* other = h->xb;
    int item = 0;
    auto tap = [&](size_t elems) -> hipError_t {
        hipError_t e = hipSuccess;
        if (h->tap_item == item && h->tap_dst)
            e = hipMemcpyAsync(h->tap_dst, cur, elems * sizeof(float), hipMemcpyDeviceToDevice, s);
        ++item;
        return e;
    };
    // sampled measurement: every prof_stride-th encode call, at most 16 calls per enable
    const bool bracket = h->profiling && (h->prof_calls++ % h->prof_stride) == 0 && h->prof_groups < h->prof_max_groups;
    if (bracket) ++h->prof_groups;
    // brackets one launch with a pair of HIP events on the stream it is launched on (sampled encode calls only)
    auto timed = [&](int kind, double work, auto&& launch) -> hipError_t {
        if (!bracket) return launch();
        if (h->ev_used == h->ev_pool.size()) {
            mnx_engine::Ev ev{};
            hipError_t e1 = hipEventCreate(&ev.a), e2 = hipEventCreate(&ev.b);
            if (e1 != hipSuccess || e2 != hipSuccess) return e1 != hipSuccess ? e1 : e2;
            h->ev_pool.push_back(ev);
        }
        mnx_engine::Ev& ev = h->ev_pool[h->ev_used++];
        ev.work = work; ev.kind = kind;
        hipError_t e0 = hipEventRecord(ev.a, s);
        if (e0 != hipSuccess) return e0;
        e0 = launch();
        if (e0 != hipSuccess) return e0;
        return hipEventRecord(ev.b, s);
    };
    const double es = (double)dt_size(dt);
    const bool split = dt_split(dt);
    // split modes: a_lo / c_lo = lo-plane offsets of the activation buffers, cls = the op class whose bit of split_mask
    // selects three product terms (default) or the hi.hi term alone (error-budget aid)
    // terms of an op class: its full count (3, or 2 for the classes of two_mask) or hi.hi alone. A 16-bit activation is
    // written as ONE plane when its consumer runs on two terms (planes_for): half the bytes out of the producer, half into
    // the consumer; the hi plane is the same bits either way.
    int stage_now = 0, block_now = 0;
    auto terms_of = [&](int cls) {
        if (!(h->split_mask & cls)) return 1;
        const bool in_range = block_now >= h->two_first[stage_now] && block_now <= h->two_last[stage_now];
        return (in_range && (h->two_mask[stage_now] & cls)) ? 2 : 3;
    };
    auto planes_for = [&](int consumer_cls) { return split && terms_of(consumer_cls) == 2 ? 1 : 2; };
    auto gemm = [&](int epi, const void* A, size_t a_lo, const W16& Wt, void* Cc, size_t c_lo, const float* bias,
                    const float* resid, int M, int N, int K, int cls, int c_planes = 2) -> hipError_t {
        SplitArgs sp;
        sp.a_lo = a_lo; sp.w_lo = Wt.lo; sp.c_lo = c_lo; sp.oscale = Wt.oscale;
        sp.terms = terms_of(cls);
        sp.c_planes = c_planes;
        // kind 4: the Linear layers of the blocks with C >= 512 (Swin-B stages 3 and 4, the MFMA-bound shapes); kind 0: the rest
        return timed((cls != SPL_MERGE && std::min(N, K) >= 512) ? 4 : 0, 2.0 * (double)M * (double)N * (double)K,
                     [&]() { return launch_gemm16(dt, epi, A, Wt.p, Cc, bias, resid, M, N, K, s, split ? &sp : nullptr); });
    };
    auto ln = [&](const float* x, const float* g, const float* b, void* y16, float* y32, int M, int Cc, int planes = 2) -> hipError_t {
        return timed(1, (double)M * Cc * (4.0 + (y16 ? es * planes / 2 : 0.0) + (y32 ? 4.0 : 0.0)),
                     [&]() { return launch_layernorm16(dt, x, g, b, y16, y32, M, Cc, 1e-5f, s, h->xn_lo, y32 ? h->enc_flag : nullptr, planes); });
    };
    if (fmt == MNX_IMG_GRAY8)
        HIPCHK(h, timed(3, (double)B * ((double)c.img_size * c.img_size + (double)Hh * Ww * C * 4.0), [&]() {
            return launch_patch_embed_gray8((const uint8_t*)images, h->pe_wt, h->pe_b, h->pe_g, h->pe_beta, cur, B, c.img_size, C, s);
        }));
    else
        HIPCHK(h, timed(3, (double)B * (3.0 * c.img_size * c.img_size + (double)Hh * Ww * C) * 4.0, [&]() {
            return launch_patch_embed((const float*)images, h->pe_wt, h->pe_b, h->pe_g, h->pe_beta, cur, B, c.img_size, C, s);
        }));
    HIPCHK(h, tap((size_t)B * Hh * Ww * C));
    for (int si = 0; si < c.n_stages; ++si) {
        StageW& st = h->stages[si];
        stage_now = si;
        const int M = B * Hh * Ww;
        for (size_t bi = 0; bi < st.blocks.size(); ++bi) {
            const BlockW& w = st.blocks[bi];
            block_now = (int)bi;
            const int shift = (bi % 2 == 0) ? 0 : c.window / 2;   // reference transformers.py:363
            HIPCHK(h, ln(cur, w.ln1_g, w.ln1_b, h->xn16, nullptr, M, C, planes_for(SPL_QKV)));
            HIPCHK(h, gemm(EPI_BIAS_16, h->xn16, h->xn_lo, w.qkv_w, h->qkv16, h->qkv_lo, w.qkv_b, nullptr, M, 3 * C, C, SPL_QKV));
            HIPCHK(h, timed(2, (double)M * C * 4.0 * es, [&]() {
                return launch_window_attn(dt, h->qkv16, w.table, h->attn16, B, Hh, Ww, C, st.heads, shift, s, h->qkv_lo,
                                          h->attn_lo, (h->split_mask & SPL_ATTN) ? 3 : 1);
            }));
            HIPCHK(h, gemm(EPI_RESID_F32, h->attn16, h->attn_lo, w.proj_w, cur, 0, w.proj_b, cur, M, C, C, SPL_PROJ));
            HIPCHK(h, ln(cur, w.ln2_g, w.ln2_b, h->xn16, nullptr, M, C, planes_for(SPL_FC1)));
            HIPCHK(h, gemm(EPI_GELU_16, h->xn16, h->xn_lo, w.fc1_w, h->h16, h->h_lo, w.fc1_b, nullptr, M, 4 * C, C, SPL_FC1, planes_for(SPL_FC2)));
            HIPCHK(h, gemm(EPI_RESID_F32, h->h16, h->h_lo, w.fc2_w, cur, 0, w.fc2_b, cur, M, C, 4 * C, SPL_FC2));
            HIPCHK(h, tap((size_t)M * C));
        }
        if (si + 1 < c.n_stages) {
            block_now = (int)st.blocks.size() - 1;        // the reduction behind the stage counts as its last block
            HIPCHK(h, launch_merge_ln16(dt, cur, st.m_g, st.m_b, h->xn16, B, Hh, Ww, C, 1e-5f, s, h->xn_lo, planes_for(SPL_MERGE)));
            HIPCHK(h, gemm(EPI_BIAS_F32, h->xn16, h->xn_lo, st.m_w, other, 0, h->zero_bias, nullptr, M / 4, 2 * C, 4 * C, SPL_MERGE));
            std::swap(cur, other);
            Hh /= 2; Ww /= 2; C *= 2;
            HIPCHK(h, tap((size_t)B * Hh * Ww * C));
        }
    }
    HIPCHK(h, ln(cur, h->fn_g, h->fn_b, nullptr, features_out, B * Hh * Ww, C));
    return MNX_OK;
}

int mnx_encode(mnx_engine* h, const float* images, int32_t B, float* features_out, void* stream) {
    return encode_impl(h, "mnx_encode", images, MNX_IMG_F32, B, features_out, stream);
}

int mnx_encode_gray8(mnx_engine* h, const uint8_t* gray, int32_t B, float* features_out, void* stream) {
    return encode_impl(h, "mnx_encode_gray8", gray, MNX_IMG_GRAY8, B, features_out, stream);
}

}  // extern "C"

namespace {

// The stream an entry point runs on, after selecting the engine's device: the caller's, or — for the legacy null stream,
// which is not capturable — the engine's own default-flag stream (created on first use), which synchronises implicitly with
// the null stream on both ends
int caller_stream(mnx_engine* h, void* stream, hipStream_t* s) {
    HIPCHK(h, hipSetDevice(h->device));
    *s = (hipStream_t)stream;
    if (!*s) {
        if (!h->own_stream) HIPCHK(h, hipStreamCreate(&h->own_stream));
        *s = h->own_stream;
    }
    return MNX_OK;
}

// A device buffer allocated by the first call that needs it and kept (allocs, bytes) until mnx_destroy
template <typename T>
int lazy_alloc(mnx_engine* h, T** p, size_t bytes) {
    if (*p) return MNX_OK;
    HIPCHK(h, hipMalloc((void**)p, bytes));
    h->allocs.push_back(*p);
    h->bytes += bytes;
    return MNX_OK;
}

// The decoder memory of n images (n <= ROW_TILE: the fp32 scratch db.memory / db.mem_kv32 holds that many) from their encoder
// features: enc_transform, then the cross-attention K / V of all layers in one SGEMM, packed into memory blocks
// blk0 .. blk0 + n - 1
int project_memory(mnx_engine* h, const float* feats, int n, int blk0, hipStream_t s) {
    const mnx_config& c = h->cfg;
    const int S = h->db.S, D = c.dec_dim;
    char* memkv = h->db.mem_kv + (size_t)blk0 * c.dec_layers * 2 * c.dec_heads * kvq_block_bytes(h->db.Sq);
    HIPCHK(h, launch_sgemm_tn(feats, h->dw.w_enc, h->dw.b_enc, h->db.memory, n * S, D, h->dw.enc_dim, s));
    HIPCHK(h, launch_sgemm_tn(h->db.memory, h->dw.w_memkv, h->dw.b_memkv, h->db.mem_kv32, n * S, c.dec_layers * 2 * D, D, s, S));
    HIPCHK(h, kvq_pack_enqueue(h->db.mem_kv32, memkv, n * c.dec_layers * 2 * c.dec_heads, S, h->db.Sq, s));
    return MNX_OK;
}

// The two encoder feature buffers of mnx_predict / mnx_predict_beam. The encoder runs ahead on enc_stream, one GROUP of up
// to `grp` reference batches (as many as max_batch holds) per buffer: it is batch-invariant, so bigger GEMM grids and fewer
// launches cost nothing. Buffer i holds the features of reference batches [first[i], first[i] + count[i]) (first -1: free).
// When a buffer counts as ready and where it is released stay with the callers.
struct FeatRing {
    mnx_engine* h;
    const void* images;                 // [n_img,3,S,S] fp32 or [n_img,S,S] gray bytes ...
    int fmt;                            // ... as MNX_IMG_* says: this struct is the one caller of the encoder
    int n_img, ref_batch, n_chunks, grp;
    int first[2] = {-1, -1}, count[2] = {0, 0};
    bool used[2] = {false, false};      // released before: a refill waits for ev_feat_free
    int next_enc = 0;                   // next reference batch to hand to the encoder

    // encode the next group into every free buffer on enc_stream; ev_enc_done[i] marks buffer i complete
    int refill() {
        const size_t img_bytes = (size_t)h->cfg.img_size * h->cfg.img_size * (fmt == MNX_IMG_GRAY8 ? 1 : 3 * sizeof(float));
        for (int i = 0; i < 2; ++i) {
            if (first[i] >= 0 || next_enc >= n_chunks) continue;
            const int cnt = std::min(grp, n_chunks - next_enc);
            const int f = next_enc * ref_batch, n = std::min(cnt * ref_batch, n_img - f);
            if (used[i]) HIPCHK(h, hipStreamWaitEvent(h->enc_stream, h->ev_feat_free[i], 0));
            MNXCHK(encode_impl(h, fmt == MNX_IMG_GRAY8 ? "mnx_encode_gray8" : "mnx_encode", (const char*)images + (size_t)f * img_bytes,
                               fmt, n, h->feat_ring[i], h->enc_stream));
            HIPCHK(h, hipEventRecord(h->ev_enc_done[i], h->enc_stream));
            first[i] = next_enc;
            count[i] = cnt;
            next_enc += cnt;
        }
        return MNX_OK;
    }
    // the buffer that holds reference batch k, -1 if none does (yet)
    int find(int k) const {
        for (int i = 0; i < 2; ++i)
            if (first[i] >= 0 && k >= first[i] && k < first[i] + count[i]) return i;
        return -1;
    }
    int end(int i) const { return first[i] + count[i]; }     // one past the last reference batch of buffer i
    const float* feats(int i, int k) const {                  // features of reference batch k (held by buffer i)
        return h->feat_ring[i] + (size_t)(k - first[i]) * ref_batch * h->db.S * h->dw.enc_dim;
    }
    // buffer i may be refilled once stream s has reached this point
    int release(int i, hipStream_t s) {
        HIPCHK(h, hipEventRecord(h->ev_feat_free[i], s));
        used[i] = true;
        first[i] = -1;
        return MNX_OK;
    }
};

// every exit path of mnx_predict*: nothing of the call may still be in flight on either stream
struct DrainGuard {
    mnx_engine* h;
    hipStream_t s;
    ~DrainGuard() { (void)hipStreamSynchronize(h->enc_stream); (void)hipStreamSynchronize(s); }
};

// row tiles of the fused greedy tick for a capacity of `rows` rows: 100 x attention tile + feed-forward tile, + 2000 for the
// mid form (0: the decoder.hip tick)
int tick_tile(const mnx_engine* h, int rows) {
    const mnx_config& c = h->cfg;
    if (c.dec_ff != 1024 || c.dec_heads != 8 || c.dec_dim != 256 || c.max_len + 1 > 512 || h->db.S > 160) return 0;
    if (h->dec_tile == 0 || rows % 16 || rows > h->db.fpart_rows) return 0;
    if (rows > h->dec_fused_max) {      // mid form: 4-row attention tiles, 16-row feed-forward tiles
        if (rows > h->dec_mid_max) return 0;
        return 2000 + 100 * 4 + 16;
    }
    const int r = h->dec_tile > 0 ? h->dec_tile : (rows <= 64 ? 2 : 4);
    return 100 * r + h->dec_tile_ff;
}

// One greedy tick on s: the begin kernel over `slots` slots, then the layers + head of `rows` rows of capacity
// (guided: the label-guided heads, reading h->guide_labels)
hipError_t enqueue_tick(mnx_engine* h, int slots, int rows, float* trace, int trace_rows, hipStream_t s, const int* forced,
                        bool guided = false) {
    return dec_enqueue_tick(h->dw, h->db, slots, rows, trace, trace_rows, s, nullptr, forced, tick_tile(h, rows),
                            guided ? h->guide_labels : nullptr, h->db.T + 2);
}

// The label table of guided decoding and what an admission of rows whose labels start at `src` installs from it
int guide_rows(mnx_engine* h, const int32_t* src, int L, int max_len, GuideRows* g) {
    MNXCHK(lazy_alloc(h, &h->guide_labels, (size_t)h->db.slots * (h->db.T + 2) * 4));
    *g = GuideRows{h->guide_labels, h->db.T + 2, src, L, std::min(L, max_len + 1)};      // max_len <= T: n + 1 <= stride
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

// The graph of one greedy tick, captured on first use and kept until mnx_destroy (null under MNX_NO_GRAPH)
int get_tick_graph(mnx_engine* h, int slots, int rows, float* trace, int trace_rows, hipStream_t s, hipGraphExec_t* out,
                   const int* forced = nullptr, bool guided = false) {
    *out = nullptr;
    if (!h->use_graph) return MNX_OK;
    // guided ticks are graphs of their own: an unguided graph is never recaptured because a guided job ran
    const GraphKey key{slots, rows, trace ? trace_rows : 0, forced ? trace_rows : 0, tick_tile(h, rows), guided ? 1 : 0};
    auto it = h->graphs.find(key);
    if (it != h->graphs.end()) { *out = it->second; return MNX_OK; }
    MNXCHK(capture_graph(h, "decode tick", s, [&]() { return enqueue_tick(h, slots, rows, trace, trace_rows, s, forced, guided); }, out));
    h->graphs[key] = *out;
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

int decode_greedy_impl(mnx_engine* h, const float* features, int32_t B, const int32_t* chunk_id, int32_t max_len,
                       int32_t stop_on_eos, const int32_t* forced_ids, int32_t* tokens, int32_t* lengths, float* token_logp,
                       float* hidden, float* logits_trace, void* stream, const int32_t* labels = nullptr, int32_t L = 0) {
    if (!h) return MNX_ERR_INVALID_ARG;
    const std::string fn = labels ? "mnx_decode_guided" : "mnx_decode_greedy";
    if (!features || !tokens || !lengths || B < 1) { h->err = fn + ": null/empty argument"; return MNX_ERR_INVALID_ARG; }
    if (B > ROW_TILE || max_len < 1 || max_len > h->cfg.max_len) {
        h->err = fn + ": B must be <= 32 and max_len <= cfg.max_len";
        return MNX_ERR_CAPACITY;
    }
    const mnx_config& c = h->cfg;
    hipStream_t s;
    MNXCHK(caller_stream(h, stream, &s));
    MNXCHK(project_memory(h, features, B, 0, s));     // memory block i = row i
    HIPCHK(h, dec_enqueue_reset(h->db, s));
    GuideRows guide{};
    if (labels) MNXCHK(guide_rows(h, labels, L, max_len, &guide));
    HIPCHK(h, dec_enqueue_admit_rows(h->db, chunk_id, B, max_len, stop_on_eos, s, labels ? &guide : nullptr));
    float* trace = nullptr;
    if (logits_trace) {
        MNXCHK(lazy_alloc(h, &h->out_trace, (size_t)c.max_len * ROW_TILE * c.vocab * 4));
        trace = h->out_trace;
    }
    const int* forced = nullptr;
    if (forced_ids) {    // teacher forcing: the caller's [B, max_len] ids, re-strided to the state's [slot][T] rows
        MNXCHK(lazy_alloc(h, &h->forced_ids, (size_t)ROW_TILE * c.max_len * 4));
        HIPCHK(h, hipMemcpy2DAsync(h->forced_ids, (size_t)h->db.T * 4, forced_ids, (size_t)max_len * 4, (size_t)max_len * 4, B,
                                   hipMemcpyDeviceToDevice, s));
        forced = h->forced_ids;
    }
    hipGraphExec_t exec = nullptr;
    const bool guided = labels != nullptr;
    MNXCHK(get_tick_graph(h, ROW_TILE, ROW_TILE, trace, B, s, &exec, forced, guided));
    MNXCHK(run_steps(h, exec, [&]() { return enqueue_tick(h, ROW_TILE, ROW_TILE, trace, B, s, forced, guided); }, ROW_TILE, max_len, s));
    HIPCHK(h, gather_enqueue(h->db, nullptr, B, max_len, tokens, lengths, token_logp, hidden, s));
    if (logits_trace) HIPCHK(h, hipMemcpyAsync(logits_trace, trace, (size_t)max_len * B * c.vocab * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return MNX_OK;
}

// kept hypotheses of all images (32 images x 8 ... 256 x 1) and how many of them one of B images may keep
constexpr int BEAM_POOL = ROW_TILE * MAX_BEAM;
inline int beam_pool_stride(int B) { return std::min(MAX_BEAM, BEAM_POOL / B); }

// The engine's beam-search buffers (allocated by the first search) set up for B images x `beam` hypotheses
int beam_buffers(mnx_engine* h, int B, int ref_batch, int beam, int n_best, bool hidden) {
    const int D = h->cfg.dec_dim, T = h->db.T;
    BeamBuffers& bm = h->beam;
    const int pool_stride = beam_pool_stride(B);
    if (pool_stride < n_best) { h->err = "beam search: n_best x images exceeds the hypothesis pool (256)"; return MNX_ERR_CAPACITY; }
    MNXCHK(lazy_alloc(h, &bm.bs, sizeof(BeamState)));
    MNXCHK(lazy_alloc(h, &bm.blp, (size_t)MAX_BEAM_IMGS * MAX_BEAM * BEAM_LP_STRIDE * 4));
    MNXCHK(lazy_alloc(h, &bm.anc, (size_t)MAX_BEAM_IMGS * MAX_BEAM * (T + 1) * 4));
    MNXCHK(lazy_alloc(h, &bm.ptok, (size_t)BEAM_POOL * T * 4));
    if (hidden) MNXCHK(lazy_alloc(h, &bm.phid, (size_t)BEAM_POOL * T * D * 4));
    bm.B = B; bm.K = beam; bm.n_best = n_best; bm.anc_stride = T + 1; bm.ref_batch = ref_batch; bm.pool_stride = pool_stride;
    return MNX_OK;
}

// Beam search over G reference batches in ONE step sequence: batch g = images [g ref_batch, (g + 1) ref_batch) of n_total
// (features at feats[g]), every image K hypotheses, one row per hypothesis — G x ref_batch x K rows per step. Images are
// independent; the positional-encoding rows are numbered inside each reference batch (beam_begin_kernel), so the result is
// that of G separate searches. Outputs [n_total, n_best, ...].
// script (mnx_decode_beam_forced; null otherwise): device [2][max_len][B][beam], the parents, then the ids, that replace every
// step's choice; logits_trace (may be null): device [max_len][B x beam][V], row (t, slot) written by the head
int decode_beam_groups(mnx_engine* h, const float* const* feats, int G, int ref_batch, int n_total, int beam, int n_best,
                       int max_len, int32_t* tokens, int32_t* lengths, float* scores, float* hidden, hipStream_t s,
                       const int* script = nullptr, float* logits_trace = nullptr) {
    const int B = n_total;
    // capacities: MAX_BEAM_IMGS images x MAX_BEAM hypotheses of state; 256 kept hypotheses (32 images x 8 ... 256 x 1)
    MNXCHK(beam_buffers(h, B, ref_batch, beam, n_best, hidden != nullptr));
    BeamBuffers run = h->beam;
    if (!hidden) run.phid = nullptr;
    if (script) { run.sc_parent = script; run.sc_token = script + (size_t)max_len * B * beam; }
    for (int g = 0; g < G; ++g)      // memory of batch g -> memory blocks g ref_batch ...
        MNXCHK(project_memory(h, feats[g], std::min(ref_batch, B - g * ref_batch), g * ref_batch, s));
    HIPCHK(h, dec_enqueue_reset(h->db, s));
    HIPCHK(h, beam_enqueue_init(h->db, run, max_len, s));
    const int rows = (B * beam + ROW_TILE - 1) / ROW_TILE * ROW_TILE;
    // one step = begin + 6 layers + head + pick, captured once per call (its arguments depend on B / beam / n_best)
    auto step = [&]() { return dec_enqueue_tick(h->dw, h->db, rows, rows, logits_trace, logits_trace ? B * beam : 0, s, &run); };
    hipGraphExec_t exec = nullptr;
    if (h->use_graph) MNXCHK(capture_graph(h, "beam step", s, step, &exec));
    struct ExecGuard {      // the per-call graph is released on every exit path
        hipGraphExec_t e;
        ~ExecGuard() { if (e) hipGraphExecDestroy(e); }
    } guard{exec};
    MNXCHK(run_steps(h, exec, step, rows, max_len, s));
    HIPCHK(h, beam_enqueue_gather(h->db, run, max_len, tokens, lengths, scores, hidden, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return MNX_OK;
}

}  // namespace

extern "C" {

int mnx_decode_greedy(mnx_engine* h, const float* features, int32_t B, const int32_t* chunk_id, int32_t max_len,
                      int32_t stop_on_eos, int32_t* tokens, int32_t* lengths, float* token_logp, float* hidden,
                      float* logits_trace, void* stream) {
    return decode_greedy_impl(h, features, B, chunk_id, max_len, stop_on_eos, nullptr, tokens, lengths, token_logp, hidden,
                              logits_trace, stream);
}

int mnx_decode_forced(mnx_engine* h, const float* features, int32_t B, const int32_t* chunk_id, int32_t max_len,
                      const int32_t* forced_ids, int32_t* argmax_ids, int32_t* lengths, float* forced_logp,
                      float* logits_trace, void* stream) {
    if (h && !forced_ids) { h->err = "mnx_decode_forced: forced_ids is null"; return MNX_ERR_INVALID_ARG; }
    return decode_greedy_impl(h, features, B, chunk_id, max_len, 1, forced_ids, argmax_ids, lengths, forced_logp, nullptr,
                              logits_trace, stream);
}

int mnx_decode_guided(mnx_engine* h, const float* features, int32_t B, const int32_t* chunk_id, int32_t max_len,
                      const int32_t* labels, int32_t L, int32_t* tokens, int32_t* lengths, float* token_logp, float* hidden,
                      float* logits_trace, void* stream) {
    if (h && (!labels || L < 2)) { h->err = "mnx_decode_guided: labels is null or L < 2"; return MNX_ERR_INVALID_ARG; }
    return decode_greedy_impl(h, features, B, chunk_id, max_len, 1, nullptr, tokens, lengths, token_logp, hidden, logits_trace,
                              stream, labels, L);
}

int mnx_decode_beam(mnx_engine* h, const float* features, int32_t B, int32_t beam, int32_t n_best, int32_t max_len,
                    int32_t* tokens, int32_t* lengths, float* scores, float* hidden, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    if (!features || !tokens || !lengths || !scores || B < 1) {
        h->err = "mnx_decode_beam: null/empty argument";
        return MNX_ERR_INVALID_ARG;
    }
    const mnx_config& c = h->cfg;
    if (B > ROW_TILE || beam < 1 || beam > MAX_BEAM || n_best < 1 || n_best > beam || max_len < 1 ||
        max_len > c.max_len || c.max_len + 1 > BEAM_ANC_MAX || c.vocab > BEAM_LP_STRIDE || B * beam > h->db.slots) {
        h->err = "mnx_decode_beam: B <= 32, 1 <= n_best <= beam <= 8, max_len <= cfg.max_len (<= 511), B x beam <= dec_slots required";
        return MNX_ERR_CAPACITY;
    }
    hipStream_t s;
    MNXCHK(caller_stream(h, stream, &s));
    return decode_beam_groups(h, &features, 1, B, B, beam, n_best, max_len, tokens, lengths, scores, hidden, s);
}

int mnx_predict_beam(mnx_engine* h, const float* images, int32_t n_img, int32_t ref_batch, int32_t beam, int32_t max_len,
                     int32_t* tokens, int32_t* lengths, float* scores, int32_t* n_atoms, int32_t* atom_idx,
                     uint8_t* edges, int32_t kmax, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    if (!images || !tokens || !lengths || !scores || !n_atoms || !atom_idx || !edges || n_img < 1) {
        h->err = "mnx_predict_beam: null/empty argument";
        return MNX_ERR_INVALID_ARG;
    }
    if (!h->have_tc) { h->err = "mnx_predict_beam: call mnx_set_token_classes first"; return MNX_ERR_INVALID_ARG; }
    const mnx_config& c = h->cfg;
    if (ref_batch < 1 || ref_batch > ROW_TILE || ref_batch > c.max_batch || beam < 1 || beam > MAX_BEAM || max_len < 1 ||
        max_len > c.max_len || kmax < 1 || kmax > h->db.kmax || c.max_len + 1 > BEAM_ANC_MAX || c.vocab > BEAM_LP_STRIDE ||
        ref_batch * beam > h->db.slots) {
        h->err = "mnx_predict_beam: ref_batch <= min(32, max_batch), beam <= 8, max_len <= cfg.max_len (<= 511), kmax <= cfg.max_atoms, "
                 "ref_batch x beam <= dec_slots required";
        return MNX_ERR_CAPACITY;
    }
    hipStream_t s;
    MNXCHK(caller_stream(h, stream, &s));
    const int D = c.dec_dim;
    // Reference batches searched together (one step sequence, decode_beam_groups): up to MNX_BEAM_GROUPS (default 8) batches
    // of one encoder launch group — a step of 4 x 160 rows costs 1.5x a step of 160 —, bounded by the state
    // capacity (MAX_BEAM_IMGS images, dec_slots rows) and by the memory blocks
    int g_max = 8;
    if (const char* e = getenv("MNX_BEAM_GROUPS")) g_max = std::max(1, atoi(e));
    g_max = std::max(1, std::min({g_max, MAX_BEAM_IMGS / ref_batch, h->db.slots / (ref_batch * beam), h->db.mem_blocks / ref_batch}));
    // decoder outputs along the winning hypotheses of the reference batches of one search
    MNXCHK(lazy_alloc(h, &h->beam_hidden, (size_t)MAX_BEAM_IMGS * c.max_len * D * 4));
    DrainGuard drain{h, s};
    // the encoder stream must not start before the caller's stream reaches this point (images ready)
    HIPCHK(h, hipMemsetAsync(h->enc_flag, 0, sizeof(int), s));     // the range flag is per call (see mnx_predict)
    HIPCHK(h, hipEventRecord(h->ev_poll[0], s));
    HIPCHK(h, hipStreamWaitEvent(h->enc_stream, h->ev_poll[0], 0));
    const int n_chunks = (n_img + ref_batch - 1) / ref_batch;
    FeatRing ring{h, images, MNX_IMG_F32, n_img, ref_batch, n_chunks, std::max(1, c.max_batch / ref_batch)};
    for (int ck = 0; ck < n_chunks;) {
        // keep both feature buffers busy on the encoder stream: the encoder of the following groups runs while the
        // beam search of these reference batches occupies the caller's stream
        MNXCHK(ring.refill());
        const int fb = ring.find(ck);
        if (fb < 0) { h->err = "mnx_predict_beam: internal: reference batch without features"; return MNX_ERR_HIP; }
        // the next G reference batches of this feature buffer, searched together
        const int G = std::min(g_max, ring.end(fb) - ck);
        const int first = ck * ref_batch, n = std::min(G * ref_batch, n_img - first);
        HIPCHK(h, hipStreamWaitEvent(s, h->ev_enc_done[fb], 0));
        const float* feats[MAX_BEAM_IMGS];
        for (int g = 0; g < G; ++g) feats[g] = ring.feats(fb, ck + g);
        int32_t* tok = tokens + (size_t)first * max_len;
        MNXCHK(decode_beam_groups(h, feats, G, ref_batch, n, beam, 1, max_len, tok, lengths + first, scores + first, h->beam_hidden, s));
        ck += G;
        if (ck == ring.end(fb)) MNXCHK(ring.release(fb, s));     // last reference batch of the group: the buffer is free again
        int32_t* aidx = atom_idx + (size_t)first * kmax;
        HIPCHK(h, atoms_enqueue_raw(h->tc_dev, tok, lengths + first, n, max_len, kmax, aidx, n_atoms + first, s));
        for (int o = 0; o < n; o += ROW_TILE) {      // the bond head's scratch holds one reference batch
            const int nb = std::min(ROW_TILE, n - o);
            HIPCHK(h, edges_enqueue(h->dw, h->db, h->beam_hidden + (size_t)o * max_len * D, nullptr, aidx + (size_t)o * kmax,
                                    n_atoms + first + o, nb, kmax, max_len, edges + (size_t)(first + o) * kmax * kmax, nullptr, s));
        }
    }
    HIPCHK(h, hipStreamSynchronize(s));
    return check_encoder_range(h, s);
}

int mnx_preprocess(mnx_engine* h, const uint8_t* rgb, int32_t height, int32_t width, int32_t pad,
                   int32_t pad_to_square, int32_t* crop_out, float* out, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    if (!rgb || !out || height < 1 || width < 1 || pad < 0) { h->err = "mnx_preprocess: null/empty argument"; return MNX_ERR_INVALID_ARG; }
    if (height > 16384 || width > 16384 || pad > 4096) { h->err = "mnx_preprocess: image larger than 16384x16384"; return MNX_ERR_CAPACITY; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, launch_preprocess(rgb, height, width, pad, pad_to_square ? 1 : 0, h->cfg.img_size, h->prep_bbox, crop_out, out,
                                (hipStream_t)stream));
    return MNX_OK;
}

int mnx_preprocess_batch(mnx_engine* h, const uint8_t* arena, const mnx_page* pages, int32_t n, int32_t max_height,
                         int32_t pad, int32_t pad_to_square, int32_t* crops_out, void* out, int32_t out_format,
                         void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    if (!arena || !pages || !out || n < 1) { h->err = "mnx_preprocess_batch: null/empty argument"; return MNX_ERR_INVALID_ARG; }
    if (out_format != MNX_IMG_F32 && out_format != MNX_IMG_GRAY8) {
        h->err = "mnx_preprocess_batch: out_format must be MNX_IMG_F32 or MNX_IMG_GRAY8";
        return MNX_ERR_INVALID_ARG;
    }
    if (max_height < 1 || max_height > 16384 || pad < 0 || pad > 4096) {
        h->err = "mnx_preprocess_batch: 1 <= max_height <= 16384 and 0 <= pad <= 4096 required";
        return MNX_ERR_INVALID_ARG;
    }
    if (((uintptr_t)arena & 15) || ((uintptr_t)pages & 7) || ((uintptr_t)out & 3) || ((uintptr_t)crops_out & 3)) {
        h->err = "mnx_preprocess_batch: arena must be 16-byte, pages 8-byte, out and crops_out 4-byte aligned";
        return MNX_ERR_INVALID_ARG;
    }
    if (n > MNX_PREP_MAX_PAGES) {
        h->err = "mnx_preprocess_batch: n " + std::to_string(n) + " exceeds MNX_PREP_MAX_PAGES = " + std::to_string(MNX_PREP_MAX_PAGES);
        return MNX_ERR_CAPACITY;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, launch_preprocess_batch(arena, pages, n, max_height, pad, pad_to_square ? 1 : 0, h->cfg.img_size,
                                      h->prep_bbox_batch, crops_out, out, out_format == MNX_IMG_GRAY8, (hipStream_t)stream));
    return MNX_OK;
}

int mnx_edges(mnx_engine* h, const float* hidden, const int32_t* atom_idx, const int32_t* n_atoms, int32_t B,
              int32_t kmax, int32_t max_len, uint8_t* edges, double* scores, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    if (!hidden || !atom_idx || !n_atoms || !edges || B < 1 || kmax < 1 || max_len < 1) {
        h->err = "mnx_edges: null/empty argument";
        return MNX_ERR_INVALID_ARG;
    }
    if (B > ROW_TILE || kmax > h->db.kmax) { h->err = "mnx_edges: B <= 32 and kmax <= cfg.max_atoms required"; return MNX_ERR_CAPACITY; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, edges_enqueue(h->dw, h->db, hidden, nullptr, atom_idx, n_atoms, B, kmax, max_len, edges, scores, (hipStream_t)stream));
    return MNX_OK;
}

// mnx_edge_probs (test aid): mnx_edges, then what edge_pair_kernel left in edge_prob for this B and kmax
int mnx_edge_probs(mnx_engine* h, const float* hidden, const int32_t* atom_idx, const int32_t* n_atoms, int32_t B,
                   int32_t kmax, int32_t max_len, uint8_t* edges, double* scores, float* probs, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    if (!hidden || !atom_idx || !n_atoms || !edges || !probs || B < 1 || kmax < 1 || max_len < 1) {
        h->err = "mnx_edge_probs: null/empty argument";
        return MNX_ERR_INVALID_ARG;
    }
    if (B > ROW_TILE || kmax > h->db.kmax) { h->err = "mnx_edge_probs: B <= 32 and kmax <= cfg.max_atoms required"; return MNX_ERR_CAPACITY; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, edges_enqueue(h->dw, h->db, hidden, nullptr, atom_idx, n_atoms, B, kmax, max_len, edges, scores, (hipStream_t)stream));
    HIPCHK(h, hipMemcpyAsync(probs, h->db.edge_prob, (size_t)B * kmax * kmax * 8 * sizeof(float), hipMemcpyDeviceToDevice,
                             (hipStream_t)stream));
    return MNX_OK;
}

int mnx_set_token_classes(mnx_engine* h, const uint8_t* flags, int32_t n, int32_t lbracket, int32_t rbracket,
                          int32_t id_C, int32_t id_l, int32_t id_B, int32_t id_r) {
    if (!h || !flags || n < 1 || n > 256) return MNX_ERR_INVALID_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    TokenClasses tc{};
    memcpy(tc.flags, flags, (size_t)n);
    tc.lbracket = lbracket; tc.rbracket = rbracket; tc.id_C = id_C; tc.id_l = id_l; tc.id_B = id_B; tc.id_r = id_r;
    tc.x0 = h->cfg.sym_offset; tc.y0 = h->cfg.sym_offset + h->cfg.coord_bins; tc.vocab = h->cfg.vocab;
    HIPCHK(h, hipMemcpy(h->tc_dev, &tc, sizeof(tc), hipMemcpyHostToDevice));
    h->have_tc = true;
    return MNX_OK;
}

int mnx_set_vocab_text(mnx_engine* h, const char* bytes, const uint32_t* offsets, int32_t n) {
    if (!h) return MNX_ERR_INVALID_ARG;
    if (!bytes || !offsets || n < 1 || n > 256) { h->err = "mnx_set_vocab_text: null pointer or n outside 1..256"; return MNX_ERR_INVALID_ARG; }
    if (n != h->cfg.sym_offset) {     // a shorter table would spell shortened SMILES without a word
        h->err = "mnx_set_vocab_text: n = " + std::to_string(n) + " names, but the vocabulary has cfg.sym_offset = " +
                 std::to_string(h->cfg.sym_offset) + " symbol ids";
        return MNX_ERR_INVALID_ARG;
    }
    if (offsets[0] != 0) { h->err = "mnx_set_vocab_text: offsets[0] must be 0"; return MNX_ERR_INVALID_ARG; }
    VocabText vt{};
    for (int i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > 8) {
            h->err = "mnx_set_vocab_text: name of id " + std::to_string(i) + " is longer than 8 bytes or its offsets decrease";
            return MNX_ERR_INVALID_ARG;
        }
        vt.len[i] = (unsigned char)(offsets[i + 1] - offsets[i]);
        memcpy(vt.name[i], bytes + offsets[i], vt.len[i]);
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy(h->vt_dev, &vt, sizeof(vt), hipMemcpyHostToDevice));
    h->have_vt = true;
    return MNX_OK;
}

// The output tables of mnx_graph_pack, mnx_expand_pack and mnx_smiles_read with their `totals`: what each tests of them
static TablesOut tables_out(mnx_mol* mols, mnx_atom* atoms, uint32_t atom_cap, mnx_bond* bonds, uint32_t bond_cap, char* text,
                            uint32_t text_cap) {
    return TablesOut{mols, (unsigned long long*)atoms, atom_cap, (unsigned long long*)bonds, bond_cap, text, text_cap};
}
static bool tables_out_null(const TablesOut& o, const uint32_t* totals) {
    return !o.mols || !totals || (!o.atoms && o.atom_cap) || (!o.bonds && o.bond_cap) || (!o.text && o.text_cap);
}
static bool tables_out_skew(const TablesOut& o, const uint32_t* totals) {
    return ((((uintptr_t)o.mols | (uintptr_t)o.atoms | (uintptr_t)o.bonds) & 7) | ((uintptr_t)totals & 3)) != 0;
}

int mnx_graph_pack(mnx_engine* h, const int32_t* tokens, const int32_t* lengths, int32_t n, int32_t T,
                   const int32_t* atom_idx, const int32_t* n_atoms, const uint8_t* edges, int32_t kmax,
                   const double* atom_scores, const double* edge_scores, const double* overall_score, mnx_mol* mols,
                   mnx_atom* atoms, uint32_t atom_cap, mnx_bond* bonds, uint32_t bond_cap, char* text, uint32_t text_cap,
                   uint32_t* totals, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    const TablesOut o = tables_out(mols, atoms, atom_cap, bonds, bond_cap, text, text_cap);
    if (!tokens || !lengths || !atom_idx || !n_atoms || !edges || tables_out_null(o, totals)) {
        h->err = "mnx_graph_pack: null pointer";
        return MNX_ERR_INVALID_ARG;
    }
    if (n < 1 || n > 65536 || T < 1 || T > 512 || kmax < 1 || kmax > h->db.kmax) {
        h->err = "mnx_graph_pack: 1 <= n <= 65536, 1 <= T <= 512 and 1 <= kmax <= cfg.max_atoms required";
        return MNX_ERR_INVALID_ARG;
    }
    const int n_scores = (atom_scores != nullptr) + (edge_scores != nullptr) + (overall_score != nullptr);
    if (n_scores != 0 && n_scores != 3) {
        h->err = "mnx_graph_pack: atom_scores, edge_scores and overall_score go together (all three or none)";
        return MNX_ERR_INVALID_ARG;
    }
    if (tables_out_skew(o, totals)) {
        h->err = "mnx_graph_pack: mols, atoms and bonds must be 8-byte aligned, totals 4-byte";
        return MNX_ERR_INVALID_ARG;
    }
    if (!h->have_tc) { h->err = "mnx_graph_pack: call mnx_set_token_classes first"; return MNX_ERR_INVALID_ARG; }
    if (!h->have_vt) { h->err = "mnx_graph_pack: call mnx_set_vocab_text first"; return MNX_ERR_INVALID_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, graph_pack_enqueue(h->tc_dev, h->vt_dev, tokens, lengths, n, T, kmax, atom_idx, n_atoms, edges, atom_scores,
                                 edge_scores, overall_score, o, totals, (hipStream_t)stream));
    return MNX_OK;
}

int mnx_set_symbol_tables(mnx_engine* h, const char* bytes, const uint32_t* offsets, const uint8_t* kinds, int32_t n) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const std::string& m) { h->err = "mnx_set_symbol_tables: " + m; return MNX_ERR_INVALID_ARG; };
    if (n < 0 || n > 512) return bad("n outside 0..512");
    if (n > 0 && (!bytes || !offsets || !kinds)) return bad("null pointer");
    if (n > 0 && offsets[0] != 0) return bad("offsets[0] must be 0");
    auto st = std::make_unique<SymbolTables>();
    memset(st.get(), 0, sizeof(SymbolTables));
    st->n = n;
    for (int i = 0; i < n; ++i) {
        if (offsets[i + 1] <= offsets[i] || offsets[i + 1] - offsets[i] > 16)
            return bad("name " + std::to_string(i) + " is empty or longer than 16 bytes, or its offsets decrease");
        if (kinds[i] != 1 && kinds[i] != 2) return bad("kinds[" + std::to_string(i) + "] must be 1 (R-group) or 2 (abbreviation)");
        st->len[i] = (unsigned char)(offsets[i + 1] - offsets[i]);
        st->kind[i] = kinds[i];
        memcpy(st->name[i], bytes + offsets[i], st->len[i]);
        if (i > 0) {        // bytewise order, a prefix in front of the longer name: what the device's binary search assumes
            const int m = std::min(st->len[i - 1], st->len[i]), c = memcmp(st->name[i - 1], st->name[i], (size_t)m);
            if (c > 0 || (c == 0 && st->len[i - 1] >= st->len[i]))
                return bad("names must be strictly ascending bytewise; name " + std::to_string(i) + " is not behind its predecessor");
        }
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy(h->st_dev, st.get(), sizeof(SymbolTables), hipMemcpyHostToDevice));
    h->have_st = true;
    h->st_n = n;
    h->have_frag = false;       // a fragment table is parallel to the names it was set for
    return MNX_OK;
}

int mnx_set_fragments(mnx_engine* h, const mnx_mol* frags, int32_t n_frags, const mnx_atom* atoms, uint32_t na, const mnx_bond* bonds,
                      uint32_t nb, const char* text, uint32_t nt, const int32_t* frag_of_name, int32_t n_names) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const std::string& m) { h->err = "mnx_set_fragments: " + m; return MNX_ERR_INVALID_ARG; };
    if (!h->have_st) return bad("call mnx_set_symbol_tables first");
    if (n_frags < 0 || n_frags > 512) return bad("n_frags outside 0..512");
    if (n_names != h->st_n) return bad("n_names must be the n of mnx_set_symbol_tables (" + std::to_string(h->st_n) + ")");
    if ((n_frags > 0 && !frags) || (na && !atoms) || (nb && !bonds) || (nt && !text) || (n_names > 0 && !frag_of_name))
        return bad("null pointer");
    // the device copy, put together on the host: bonds sorted by (i, j), every fragment's symbols behind one another
    std::vector<FragRec> rec((size_t)n_frags);
    std::vector<unsigned> fa, fb;
    std::vector<unsigned char> ft;
    for (int f = 0; f < n_frags; ++f) {
        const mnx_mol& m = frags[f];
        const std::string who = "fragment " + std::to_string(f);
        if (m.n_atoms < 1 || m.n_atoms > 32) return bad(who + " has " + std::to_string(m.n_atoms) + " atoms; 1 to 32 required");
        if ((uint64_t)m.atom0 + m.n_atoms > na || (uint64_t)m.bond0 + m.n_bonds > nb || (uint64_t)m.text0 + m.smiles_len > nt)
            return bad(who + ": its records end behind a table");
        FragRec& r = rec[(size_t)f];
        r.atom0 = (unsigned)fa.size(); r.bond0 = (unsigned)fb.size(); r.text0 = (unsigned)ft.size();
        r.n_atoms = (unsigned short)m.n_atoms;
        unsigned len = 0;
        for (uint32_t a = 0; a < m.n_atoms; ++a) {
            const mnx_atom& x = atoms[m.atom0 + a];
            if (x.sym_len < 1 || x.sym_len > 8) return bad(who + ", atom " + std::to_string(a) + ": a symbol has 1 to 8 bytes");
            if ((uint64_t)m.text0 + x.sym0 + x.sym_len > nt) return bad(who + ", atom " + std::to_string(a) + ": its symbol ends behind the text");
            fa.push_back(len | (unsigned)x.sym_len << 16);
            ft.insert(ft.end(), (const unsigned char*)text + m.text0 + x.sym0, (const unsigned char*)text + m.text0 + x.sym0 + x.sym_len);
            len += x.sym_len;
        }
        r.text_len = (unsigned short)len;
        std::vector<unsigned> own;
        for (uint32_t k = 0; k < m.n_bonds; ++k) {
            const mnx_bond& x = bonds[m.bond0 + k];
            const std::string which = who + ", bond " + std::to_string(k);
            if (!(x.i < x.j && x.j < m.n_atoms)) return bad(which + ": i < j < n_atoms required");
            if (x.type < 1 || x.type > 4 || x.rev != x.type) return bad(which + ": type 1 to 4 and rev == type required");
            own.push_back((unsigned)x.i | (unsigned)x.j << 8 | (unsigned)x.type << 16);
        }
        std::sort(own.begin(), own.end(), [](unsigned p, unsigned q) { return ((p & 0xff) << 8 | (p >> 8 & 0xff)) < ((q & 0xff) << 8 | (q >> 8 & 0xff)); });
        unsigned n0 = 0;
        for (size_t k = 0; k < own.size(); ++k) {
            if (k > 0 && (own[k] & 0xffff) == (own[k - 1] & 0xffff)) return bad(who + ": the same pair of atoms in two bonds");
            n0 += (own[k] & 0xff) == 0;
        }
        r.n_bonds = (unsigned short)own.size();
        r.n_bonds0 = (unsigned short)n0;
        fb.insert(fb.end(), own.begin(), own.end());
    }
    std::vector<unsigned char> kinds((size_t)std::max(n_names, 1));
    {   // the kinds as the device holds them
        auto st = std::make_unique<SymbolTables>();
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, hipMemcpy(st.get(), h->st_dev, sizeof(SymbolTables), hipMemcpyDeviceToHost));
        memcpy(kinds.data(), st->kind, (size_t)n_names);
    }
    for (int k = 0; k < n_names; ++k) {
        if (frag_of_name[k] < -1 || frag_of_name[k] >= n_frags) return bad("frag_of_name[" + std::to_string(k) + "] outside -1.." + std::to_string(n_frags - 1));
        if (frag_of_name[k] >= 0 && kinds[(size_t)k] != 2) return bad("frag_of_name[" + std::to_string(k) + "]: only an abbreviation (kind 2) takes a fragment");
    }
    // one allocation: frag_of_name | records | atoms | bonds | text, each part 8-byte aligned
    auto up8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
    const size_t o_rec = up8((size_t)std::max(n_names, 1) * sizeof(int)), o_atoms = o_rec + up8(std::max(rec.size(), (size_t)1) * sizeof(FragRec));
    const size_t o_bonds = o_atoms + up8(std::max(fa.size(), (size_t)1) * 4), o_text = o_bonds + up8(std::max(fb.size(), (size_t)1) * 4);
    const size_t total = o_text + up8(std::max(ft.size(), (size_t)1));
    std::vector<unsigned char> blob(total, 0);
    if (n_names) memcpy(blob.data(), frag_of_name, (size_t)n_names * sizeof(int));
    if (!rec.empty()) memcpy(blob.data() + o_rec, rec.data(), rec.size() * sizeof(FragRec));
    if (!fa.empty()) memcpy(blob.data() + o_atoms, fa.data(), fa.size() * 4);
    if (!fb.empty()) memcpy(blob.data() + o_bonds, fb.data(), fb.size() * 4);
    if (!ft.empty()) memcpy(blob.data() + o_text, ft.data(), ft.size());
    void* dev = nullptr;
    HIPCHK(h, hipMalloc(&dev, total));
    if (hipError_t e = hipMemcpy(dev, blob.data(), total, hipMemcpyHostToDevice); e != hipSuccess) {
        hipFree(dev);
        h->err = std::string("mnx_set_fragments: hipMemcpy: ") + hipGetErrorString(e);
        return MNX_ERR_HIP;
    }
    if (h->frag_dev) {          // an earlier table may still be read by launches in flight
        (void)hipDeviceSynchronize();
        hipFree(h->frag_dev);
    }
    h->frag_dev = dev;
    const unsigned char* d = (const unsigned char*)dev;
    h->fv = FragView{(const int*)d, (const FragRec*)(d + o_rec), (const unsigned*)(d + o_atoms), (const unsigned*)(d + o_bonds), d + o_text};
    h->have_frag = true;
    return MNX_OK;
}

// What mnx_molfile_pack, mnx_expand_pack, mnx_normalize_pack, mnx_kekulize_pack and the five mnx_smiles_pack* test before they launch, in
// the order in which a call refused for two reasons reports them. Its own pointers (outs_null, outs_skew) the entry point tests; `aligned` ends its alignment message.
static int check_packed_tables(mnx_engine* h, const char* fn, const PackedTables& t, bool outs_null, bool outs_skew,
                               const char* aligned, bool reads_symbols = true) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const std::string& m) { h->err = std::string(fn) + ": " + m; return MNX_ERR_INVALID_ARG; };
    if (!t.mols || (!t.atoms && t.n_atom_records) || (!t.bonds && t.n_bond_records) || (!t.text && t.n_text_bytes) || outs_null)
        return bad("null pointer");
    if (t.n < 1 || t.n > 65536) return bad("1 <= n <= 65536 required");
    if ((((uintptr_t)t.mols | (uintptr_t)t.atoms | (uintptr_t)t.bonds) & 7) || outs_skew)
        return bad(std::string("mols, atoms and bonds must be 8-byte aligned, ") + aligned);
    if (reads_symbols && !h->have_st) return bad("call mnx_set_symbol_tables first");
    return MNX_OK;
}

int mnx_molfile_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                     const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes,
                     const int32_t* scale, mnx_molfile* files, char* out, uint32_t out_cap, uint32_t* totals, void* stream) {
    const PackedTables t{mols, n, atoms, n_atom_records, bonds, n_bond_records, (const unsigned char*)text, n_text_bytes};
    if (int rc = check_packed_tables(h, "mnx_molfile_pack", t, !files || !totals || (!out && out_cap),
                                     (((uintptr_t)files | (uintptr_t)totals | (uintptr_t)scale) & 3) != 0, "files, scale and totals 4-byte"))
        return rc;
    if (h->cfg.coord_bins < 2) { h->err = "mnx_molfile_pack: cfg.coord_bins must be at least 2"; return MNX_ERR_INVALID_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, molfile_pack_enqueue(h->st_dev, t, scale, h->cfg.coord_bins, files, out, out_cap, totals, (hipStream_t)stream));
    return MNX_OK;
}

// mnx_expand_pack and mnx_formula_pack (formula, with its max_steps): one check, one way to the pass's three launches
static int grow_pack(mnx_engine* h, const char* fn, const PackedTables& t, const TablesOut& o, uint16_t* origin, uint32_t* totals,
                     void* stream, bool formula = false, uint32_t max_steps = 0) {
    if (int rc = check_packed_tables(h, fn, t, tables_out_null(o, totals), tables_out_skew(o, totals) || ((uintptr_t)origin & 1) != 0,
                                     "the output tables too, totals 4-byte, origin 2-byte"))
        return rc;
    if (!h->have_frag) { h->err = std::string(fn) + ": call mnx_set_fragments first"; return MNX_ERR_INVALID_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    if (formula) HIPCHK(h, formula_pack_enqueue(h->st_dev, h->fv, t, o, origin, totals, max_steps, (hipStream_t)stream));
    else HIPCHK(h, expand_pack_enqueue(h->st_dev, h->fv, t, o, origin, totals, (hipStream_t)stream));
    return MNX_OK;
}

int mnx_expand_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                    const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_mol* mols_out,
                    mnx_atom* atoms_out, uint32_t atom_cap, mnx_bond* bonds_out, uint32_t bond_cap, char* text_out, uint32_t text_cap,
                    uint16_t* origin, uint32_t* totals, void* stream) {
    const PackedTables t{mols, n, atoms, n_atom_records, bonds, n_bond_records, (const unsigned char*)text, n_text_bytes};
    const TablesOut o = tables_out(mols_out, atoms_out, atom_cap, bonds_out, bond_cap, text_out, text_cap);
    return grow_pack(h, "mnx_expand_pack", t, o, origin, totals, stream);
}

int mnx_formula_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                     const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_mol* mols_out,
                     mnx_atom* atoms_out, uint32_t atom_cap, mnx_bond* bonds_out, uint32_t bond_cap, char* text_out, uint32_t text_cap,
                     uint16_t* origin, uint32_t* totals, uint32_t max_steps, void* stream) {
    const PackedTables t{mols, n, atoms, n_atom_records, bonds, n_bond_records, (const unsigned char*)text, n_text_bytes};
    const TablesOut o = tables_out(mols_out, atoms_out, atom_cap, bonds_out, bond_cap, text_out, text_cap);
    return grow_pack(h, "mnx_formula_pack", t, o, origin, totals, stream, true, max_steps);
}

// mnx_main_pack reads no symbol: it needs neither symbol tables nor fragments
int mnx_main_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                  const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_mol* mols_out,
                  mnx_atom* atoms_out, uint32_t atom_cap, mnx_bond* bonds_out, uint32_t bond_cap, char* text_out, uint32_t text_cap,
                  uint16_t* origin, uint32_t* totals, void* stream) {
    const PackedTables t{mols, n, atoms, n_atom_records, bonds, n_bond_records, (const unsigned char*)text, n_text_bytes};
    const TablesOut o = tables_out(mols_out, atoms_out, atom_cap, bonds_out, bond_cap, text_out, text_cap);
    if (int rc = check_packed_tables(h, "mnx_main_pack", t, tables_out_null(o, totals), tables_out_skew(o, totals) || ((uintptr_t)origin & 1) != 0,
                                     "the output tables too, totals 4-byte, origin 2-byte", false))
        return rc;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, main_pack_enqueue(t, o, origin, totals, (hipStream_t)stream));
    return MNX_OK;
}

// mnx_normalize_pack and mnx_kekulize_pack (kekulize, with its max_steps): one check, one way to the pass's three launches
static int respell_pack(mnx_engine* h, const char* fn, const PackedTables& t, const TablesOut& o, uint8_t* atom_notes, uint32_t* totals,
                        void* stream, bool kekulize = false, uint32_t max_steps = 0) {
    if (int rc = check_packed_tables(h, fn, t, tables_out_null(o, totals), tables_out_skew(o, totals), "the output tables too, totals 4-byte"))
        return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if (kekulize) HIPCHK(h, kekulize_pack_enqueue(h->st_dev, t, o, atom_notes, totals, max_steps, (hipStream_t)stream));
    else HIPCHK(h, normalize_pack_enqueue(h->st_dev, t, o, atom_notes, totals, (hipStream_t)stream));
    return MNX_OK;
}

int mnx_normalize_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                       const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_mol* mols_out,
                       mnx_atom* atoms_out, uint32_t atom_cap, mnx_bond* bonds_out, uint32_t bond_cap, char* text_out,
                       uint32_t text_cap, uint8_t* atom_notes, uint32_t* totals, void* stream) {
    const PackedTables t{mols, n, atoms, n_atom_records, bonds, n_bond_records, (const unsigned char*)text, n_text_bytes};
    const TablesOut o = tables_out(mols_out, atoms_out, atom_cap, bonds_out, bond_cap, text_out, text_cap);
    return respell_pack(h, "mnx_normalize_pack", t, o, atom_notes, totals, stream);
}

int mnx_kekulize_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                      const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_mol* mols_out,
                      mnx_atom* atoms_out, uint32_t atom_cap, mnx_bond* bonds_out, uint32_t bond_cap, char* text_out,
                      uint32_t text_cap, uint8_t* atom_notes, uint32_t* totals, uint32_t max_steps, void* stream) {
    const PackedTables t{mols, n, atoms, n_atom_records, bonds, n_bond_records, (const unsigned char*)text, n_text_bytes};
    const TablesOut o = tables_out(mols_out, atoms_out, atom_cap, bonds_out, bond_cap, text_out, text_cap);
    return respell_pack(h, "mnx_kekulize_pack", t, o, atom_notes, totals, stream, true, max_steps);
}

int mnx_smiles_read(mnx_engine* h, const char* bytes, uint32_t n_bytes, const uint32_t* offsets, int32_t n, mnx_mol* mols,
                    mnx_read* recs, mnx_atom* atoms, uint32_t atom_cap, mnx_bond* bonds, uint32_t bond_cap, char* text,
                    uint32_t text_cap, uint32_t* totals, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const char* m) { h->err = std::string("mnx_smiles_read: ") + m; return MNX_ERR_INVALID_ARG; };
    const TablesOut o = tables_out(mols, atoms, atom_cap, bonds, bond_cap, text, text_cap);
    if ((!bytes && n_bytes) || !offsets || !recs || tables_out_null(o, totals)) return bad("null pointer");
    if (n < 1 || n > 65536) return bad("1 <= n <= 65536 required");
    if (tables_out_skew(o, totals) || (((uintptr_t)recs | (uintptr_t)offsets) & 3))
        return bad("mols, atoms and bonds must be 8-byte aligned, recs, offsets and totals 4-byte");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, smiles_read_enqueue((const unsigned char*)bytes, n_bytes, offsets, n, recs, o, totals, (hipStream_t)stream));
    return MNX_OK;
}

int mnx_molfile_read(mnx_engine* h, const char* bytes, uint32_t n_bytes, const uint32_t* offsets, int32_t n,
                     const int32_t* scale, int32_t fit, mnx_mol* mols, mnx_molread* recs, mnx_atom* atoms, uint32_t atom_cap,
                     mnx_bond* bonds, uint32_t bond_cap, char* text, uint32_t text_cap, uint32_t* totals, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const char* m) { h->err = std::string("mnx_molfile_read: ") + m; return MNX_ERR_INVALID_ARG; };
    const TablesOut o = tables_out(mols, atoms, atom_cap, bonds, bond_cap, text, text_cap);
    if ((!bytes && n_bytes) || !offsets || !recs || tables_out_null(o, totals)) return bad("null pointer");
    if (n < 1 || n > 65536) return bad("1 <= n <= 65536 required");
    if (fit != 0 && fit != 1) return bad("fit must be 0 or 1");
    if (fit && scale) return bad("fit = 1 takes no scale");
    if (tables_out_skew(o, totals) || (((uintptr_t)recs | (uintptr_t)offsets | (uintptr_t)scale) & 3))
        return bad("mols, atoms and bonds must be 8-byte aligned, recs, offsets, scale and totals 4-byte");
    if (h->cfg.coord_bins < 2) return bad("cfg.coord_bins must be at least 2");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, molfile_read_enqueue((const unsigned char*)bytes, n_bytes, offsets, n, scale, fit, (unsigned)h->cfg.coord_bins - 1u, recs, o,
                                   totals, (hipStream_t)stream));
    return MNX_OK;
}

// mnx_smiles_pack, mnx_smiles_pack_stereo, mnx_smiles_pack_marks, mnx_smiles_pack_canonical and mnx_smiles_pack_symmetric: one
// check, one enqueue path, a pair of kernels per set of marks; canonical: on the ranks that one more kernel in front of them
// leaves in `rank`; symmetric: canonical with the symmetry rule, which needs `sym_class` too
static int smiles_pack(mnx_engine* h, const char* fn, uint32_t marks, const PackedTables& t, mnx_smiles* recs, uint16_t* order,
                       char* out, uint32_t out_cap, uint32_t* totals, void* stream, bool canonical = false, uint16_t* rank = nullptr,
                       uint16_t* sym_class = nullptr, bool symmetric = false, uint8_t* atom_marks = nullptr) {
    if (int rc = check_packed_tables(h, fn, t, !recs || !totals || (!out && out_cap) || (canonical && !rank) || (symmetric && !sym_class),
                                     (((uintptr_t)recs | (uintptr_t)totals) & 3) != 0 ||
                                         (((uintptr_t)order | (uintptr_t)rank | (uintptr_t)sym_class) & 1) != 0,
                                     canonical ? "recs and totals 4-byte, order, rank and sym_class 2-byte" : "recs and totals 4-byte, order 2-byte"))
        return rc;
    if (marks & ~(MNX_SMILES_MARK_TETRAHEDRAL | MNX_SMILES_MARK_DOUBLE_BOND)) {
        h->err = std::string(fn) + ": marks may hold MNX_SMILES_MARK_TETRAHEDRAL and MNX_SMILES_MARK_DOUBLE_BOND only";
        return MNX_ERR_INVALID_ARG;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, smiles_pack_enqueue(h->st_dev, t, marks, recs, order, rank, sym_class, out, out_cap, totals, (hipStream_t)stream, symmetric,
                                  atom_marks));
    return MNX_OK;
}

int mnx_smiles_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                    const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_smiles* recs,
                    uint16_t* order, char* out, uint32_t out_cap, uint32_t* totals, void* stream) {
    const PackedTables t{mols, n, atoms, n_atom_records, bonds, n_bond_records, (const unsigned char*)text, n_text_bytes};
    return smiles_pack(h, "mnx_smiles_pack", 0u, t, recs, order, out, out_cap, totals, stream);
}

int mnx_smiles_pack_stereo(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                           const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes,
                           mnx_smiles* recs, uint16_t* order, char* out, uint32_t out_cap, uint32_t* totals, void* stream) {
    const PackedTables t{mols, n, atoms, n_atom_records, bonds, n_bond_records, (const unsigned char*)text, n_text_bytes};
    return smiles_pack(h, "mnx_smiles_pack_stereo", MNX_SMILES_MARK_TETRAHEDRAL, t, recs, order, out, out_cap, totals, stream);
}

int mnx_smiles_pack_marks(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                          const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes,
                          mnx_smiles* recs, uint16_t* order, char* out, uint32_t out_cap, uint32_t* totals, uint32_t marks,
                          void* stream) {
    const PackedTables t{mols, n, atoms, n_atom_records, bonds, n_bond_records, (const unsigned char*)text, n_text_bytes};
    return smiles_pack(h, "mnx_smiles_pack_marks", marks, t, recs, order, out, out_cap, totals, stream);
}

int mnx_smiles_pack_canonical(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                              const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes,
                              mnx_smiles* recs, uint16_t* order, uint16_t* rank, uint16_t* sym_class, char* out,
                              uint32_t out_cap, uint32_t* totals, uint32_t marks, void* stream) {
    const PackedTables t{mols, n, atoms, n_atom_records, bonds, n_bond_records, (const unsigned char*)text, n_text_bytes};
    return smiles_pack(h, "mnx_smiles_pack_canonical", marks, t, recs, order, out, out_cap, totals, stream, true, rank, sym_class);
}

int mnx_smiles_pack_symmetric(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                              const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes,
                              mnx_smiles* recs, uint16_t* order, uint16_t* rank, uint16_t* sym_class, uint8_t* atom_marks,
                              char* out, uint32_t out_cap, uint32_t* totals, uint32_t marks, void* stream) {
    const PackedTables t{mols, n, atoms, n_atom_records, bonds, n_bond_records, (const unsigned char*)text, n_text_bytes};
    return smiles_pack(h, "mnx_smiles_pack_symmetric", marks, t, recs, order, out, out_cap, totals, stream, true, rank, sym_class,
                       true, atom_marks);
}

int mnx_fingerprint_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                         const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_fp* recs,
                         uint32_t* bits, uint32_t max_bonds, uint32_t max_steps, void* stream) {
    const PackedTables t{mols, n, atoms, n_atom_records, bonds, n_bond_records, (const unsigned char*)text, n_text_bytes};
    if (int rc = check_packed_tables(h, "mnx_fingerprint_pack", t, !recs || !bits, (((uintptr_t)recs | (uintptr_t)bits) & 3) != 0,
                                     "recs and bits 4-byte"))
        return rc;
    if (max_bonds > MNX_FP_MAX_BONDS) { h->err = "mnx_fingerprint_pack: max_bonds must be 1 to 7, or 0 for 7"; return MNX_ERR_INVALID_ARG; }
    if (max_steps > MNX_FP_MAX_STEPS) {
        h->err = "mnx_fingerprint_pack: max_steps must not exceed MNX_FP_MAX_STEPS (1048576)";
        return MNX_ERR_INVALID_ARG;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, fingerprint_pack_enqueue(h->st_dev, t, recs, bits, max_bonds ? max_bonds : MNX_FP_MAX_BONDS,
                                       max_steps ? max_steps : MNX_FP_DEFAULT_STEPS, (hipStream_t)stream));
    return MNX_OK;
}

int mnx_tanimoto(mnx_engine* h, const uint32_t* a, const uint32_t* b, int32_t n, uint32_t* both, uint32_t* either,
                 double* similarity, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const char* m) { h->err = std::string("mnx_tanimoto: ") + m; return MNX_ERR_INVALID_ARG; };
    if (!a || !b) return bad("null pointer");
    if (!both && !either && !similarity) return bad("both, either and similarity are all null");
    if (n < 1 || n > 65536) return bad("1 <= n <= 65536 required");
    if ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)both | (uintptr_t)either) & 3) || ((uintptr_t)similarity & 7))
        return bad("a, b, both and either must be 4-byte aligned, similarity 8-byte");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, tanimoto_enqueue(a, b, n, both, either, similarity, (hipStream_t)stream));
    return MNX_OK;
}

int mnx_atom_scan(mnx_engine* h, const int32_t* tokens, const int32_t* lengths, int32_t n, int32_t T, int32_t kmax,
                  int32_t* atom_idx, int32_t* n_atoms, void* stream) {
    if (!h || !tokens || !lengths || !atom_idx || !n_atoms || n < 1 || T < 1 || kmax < 1) return MNX_ERR_INVALID_ARG;
    if (!h->have_tc) { h->err = "mnx_atom_scan: call mnx_set_token_classes first"; return MNX_ERR_INVALID_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, atoms_enqueue_raw(h->tc_dev, tokens, lengths, n, T, kmax, atom_idx, n_atoms, (hipStream_t)stream));
    return MNX_OK;
}

int mnx_confidence(mnx_engine* h, const int32_t* tokens, const int32_t* lengths, const float* token_logp, int32_t n,
                   int32_t T, const int32_t* atom_idx, const int32_t* n_atoms, const double* edge_scores, int32_t kmax,
                   double* atom_scores, double* overall_score, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    if (!tokens || !lengths || !token_logp || !atom_idx || !n_atoms || !edge_scores || !atom_scores || !overall_score ||
        n < 1 || T < 1 || kmax < 1) {
        h->err = "mnx_confidence: null/empty argument";
        return MNX_ERR_INVALID_ARG;
    }
    if (!h->have_tc) { h->err = "mnx_confidence: call mnx_set_token_classes first"; return MNX_ERR_INVALID_ARG; }
    if (T > 512 || kmax > h->db.kmax) { h->err = "mnx_confidence: T <= 512 and kmax <= cfg.max_atoms required"; return MNX_ERR_CAPACITY; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, confidence_enqueue_raw(h->tc_dev, tokens, lengths, token_logp, n, T, kmax, atom_idx, n_atoms, edge_scores,
                                     atom_scores, overall_score, (hipStream_t)stream));
    return MNX_OK;
}

}  // extern "C"

namespace {
// outputs of mnx_predict_confidence, per image (token_logp may be null)
struct ConfOut {
    float* token_logp;
    double *edge_scores, *atom_scores, *overall;
};
}  // namespace

// The whole hot path for n_img images with continuous batching (see include/molnextr_hip.h): the body of mnx_predict and,
// with `conf`, of mnx_predict_confidence. Without `conf` it enqueues exactly mnx_predict's launches.
static int predict_impl(mnx_engine* h, const char* name, const void* images, int img_fmt, int32_t n_img, int32_t ref_batch,
                        int32_t max_len, int32_t stop_on_eos, int32_t* tokens, int32_t* lengths, int32_t* n_atoms,
                        int32_t* atom_idx, uint8_t* edges, int32_t kmax, const ConfOut* conf, void* stream,
                        const int32_t* labels = nullptr, int32_t L = 0) {
    if (!h) return MNX_ERR_INVALID_ARG;
    if (!images || !tokens || !lengths || !n_atoms || !atom_idx || !edges || n_img < 1 ||
        (conf && (!conf->edge_scores || !conf->atom_scores || !conf->overall))) {
        h->err = std::string(name) + ": null/empty argument";
        return MNX_ERR_INVALID_ARG;
    }
    if (img_fmt == MNX_IMG_GRAY8 && ((uintptr_t)images & 3)) { h->err = std::string(name) + ": gray must be 4-byte aligned"; return MNX_ERR_INVALID_ARG; }
    if (!h->have_tc) { h->err = std::string(name) + ": call mnx_set_token_classes first"; return MNX_ERR_INVALID_ARG; }
    const mnx_config& c = h->cfg;
    const int SL = h->db.slots;
    {   // a reference batch is decoded as ONE chunk (its PE numbering spans all of its rows): it must fit every bound at once
        const char* hit = ref_batch > MAX_REF_BATCH ? "MAX_REF_BATCH" : ref_batch > c.max_batch ? "cfg.max_batch"
                        : ref_batch > SL ? "cfg.dec_slots" : ref_batch > c.pe_len ? "cfg.pe_len" : nullptr;
        const int lim = ref_batch > MAX_REF_BATCH ? MAX_REF_BATCH : ref_batch > c.max_batch ? c.max_batch
                      : ref_batch > SL ? SL : c.pe_len;
        if (hit) {
            h->err = std::string(name) + ": ref_batch " + std::to_string(ref_batch) + " exceeds " + hit + " = " +
                     std::to_string(lim);
            return MNX_ERR_CAPACITY;
        }
    }
    if (ref_batch < 1 || max_len < 1 || max_len > c.max_len || kmax < 1 || kmax > h->db.kmax) {
        h->err = std::string(name) + ": 1 <= ref_batch, max_len <= cfg.max_len, kmax <= cfg.max_atoms required";
        return MNX_ERR_CAPACITY;
    }
    hipStream_t s;
    MNXCHK(caller_stream(h, stream, &s));
    const bool guided = labels != nullptr;      // label-guided: rows carry labels [n_img, L] (mnx_predict_guided)
    GuideRows guide{};
    if (guided) MNXCHK(guide_rows(h, labels, L, max_len, &guide));
    const int n_chunks = (n_img + ref_batch - 1) / ref_batch;
    // A chunk (one reference batch) holds ceil(n / 32) row tiles, not necessarily contiguous; tile j holds its rows
    // 32 j .. 32 j + 31 in slots tile * 32 + i, memory K/V blocks likewise, and its slot list at slot_lists[tile]. The chunk's
    // tag (the PE numbering unit of dec_begin_kernel, the index of its alive counter) is its first tile: tags < MAX_CHUNKS.
    struct Chunk { int first, n, tag, admit_seq; std::vector<int> tiles; };
    std::vector<Chunk> live;
    std::vector<int> free_tiles;
    for (int i = h->n_chunk_bufs - 1; i >= 0; --i) free_tiles.push_back(i);
    int* pinned = h->host_flag;                       // [2][1 + MAX_CHUNKS] snapshots, then slot lists per tile
    int* pin_slots = h->host_flag + 2 * (1 + MAX_CHUNKS);
    int bound = 0;                                    // upper bound of alive rows (host-side, conservative)
    std::vector<std::pair<int, int>> admits;          // (iteration, rows) of every admission
    HIPCHK(h, dec_enqueue_reset(h->db, s));
    // the range flag is per call: an earlier mnx_encode on a bad input (whose caller did not poll mnx_encoder_status) must
    // not make THIS job report MNX_ERR_RANGE
    HIPCHK(h, hipMemsetAsync(h->enc_flag, 0, sizeof(int), s));
    // the encoder stream must not start before the caller's stream reaches this point (images ready)
    HIPCHK(h, hipEventRecord(h->ev_poll[0], s));
    HIPCHK(h, hipStreamWaitEvent(h->enc_stream, h->ev_poll[0], 0));
    int next = 0, done = 0, seq = 0;
    const char* trace_path = getenv("MNX_TRACE");
    FILE* tf = trace_path ? fopen(trace_path, "a") : nullptr;
    const std::unique_ptr<FILE, int (*)(FILE*)> tf_close(tf, fclose);   // closed on every exit path, after the drain
    DrainGuard drain{h, s};
    auto now_ms = []() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; };
    const double t_begin = now_ms();
    double host_wait_ms = 0.0;
    // each reference batch of an encoder group is admitted on its own
    FeatRing ring{h, images, img_fmt, n_img, ref_batch, n_chunks, std::max(1, c.max_batch / ref_batch)};
    const int ticks_per_poll = 4;            // measured: 2-4 equal, 8 = -4 % (retirement lags)
    while (done < n_chunks) {
        // ---- encoder prefetch: keep both feature buffers busy on the encoder stream
        MNXCHK(ring.refill());
        // ---- admission (in image order): only once the chunk's features are READY, so the decode stream never
        //      waits for the encoder; project the memory and admit on the decode stream
        while (next < n_chunks) {
            const int fb = ring.find(next);
            if (fb < 0) break;
            const int first = next * ref_batch, n = std::min(ref_batch, n_img - first);
            const int n_tiles = (n + ROW_TILE - 1) / ROW_TILE;
            if ((int)free_tiles.size() < n_tiles) break;   // every row of a batch starts at step 0 together: wait for all tiles
            // nothing to decode: wait for the features instead of polling
            const bool idle = live.empty();
            hipError_t q = idle ? hipEventSynchronize(h->ev_enc_done[fb]) : hipEventQuery(h->ev_enc_done[fb]);
            if (q == hipErrorNotReady) break;
            if (q != hipSuccess) { h->err = std::string("encoder event: ") + hipGetErrorString(q); return MNX_ERR_HIP; }
            Chunk ck;
            ck.first = first; ck.n = n; ck.admit_seq = seq;
            for (int j = 0; j < n_tiles; ++j) { ck.tiles.push_back(free_tiles.back()); free_tiles.pop_back(); }
            ck.tag = ck.tiles[0];
            HIPCHK(h, hipStreamWaitEvent(s, h->ev_enc_done[fb], 0));   // already complete: ordering only
            // memory projection tile by tile: the fp32 scratch (db.memory, db.mem_kv32) holds 32 rows
            for (int j = 0; j < n_tiles; ++j) {
                const float* feats = ring.feats(fb, next) + (size_t)j * ROW_TILE * h->db.S * h->dw.enc_dim;
                MNXCHK(project_memory(h, feats, std::min(ROW_TILE, n - j * ROW_TILE), ck.tiles[j] * ROW_TILE, s));
            }
            if (next + 1 == ring.end(fb)) MNXCHK(ring.release(fb, s));   // last reference batch of the group: buffer is free again
            // every tile of the chunk is admitted before the next tick, rows 32 j + i under the chunk's one tag
            for (int j = 0; j < n_tiles; ++j) {
                const int tile = ck.tiles[j], nj = std::min(ROW_TILE, n - j * ROW_TILE);
                int* sl_dev = h->slot_lists + (size_t)tile * ROW_TILE;
                int* sl_pin = pin_slots + (size_t)tile * ROW_TILE;     // pinned, private to this tile until its chunk retires
                for (int i = 0; i < nj; ++i) sl_pin[i] = tile * ROW_TILE + i;
                HIPCHK(h, hipMemcpyAsync(sl_dev, sl_pin, (size_t)nj * 4, hipMemcpyHostToDevice, s));
                guide.src = guided ? labels + (size_t)(first + j * ROW_TILE) * L : nullptr;     // labels travel with their rows
                HIPCHK(h, dec_enqueue_admit(h->db, sl_dev, h->rowc_seq + j * ROW_TILE, nj, ck.tag, tile * ROW_TILE, max_len,
                                            stop_on_eos ? 1 : 0, s, guided ? &guide : nullptr));
            }
            bound += n;
            admits.emplace_back(seq, n);
            live.push_back(std::move(ck));
            ++next;
        }
        if (live.empty()) continue;       // (only possible before the first admission)
        // ---- a group of ticks, then a status snapshot
        // launch the tick graph sized for the alive-row bound (dense active list: idle row tiles are not launched)
        // (one graph per capacity, captured on first use: multiples of 64 up to 1024 rows, of 128 up to 2048, of 256 beyond)
        const int cap_step = bound <= 1024 ? 64 : bound <= 2048 ? 128 : 256;
        const int rows_cap = std::min(SL, (std::max(bound, 1) + cap_step - 1) / cap_step * cap_step);
        // the begin kernel scans slot tiles 0 .. highest live tile only (tiles are handed out lowest-first): a 20-batch job
        // keeps it to 1024 of the 3072 slots — one pass of its 1024 threads instead of three; steps of 1024 keep the number of
        // tick graphs (one per scan range and capacity) small
        int hi_tile = 0;
        for (const Chunk& ck : live)
            for (int t : ck.tiles) hi_tile = std::max(hi_tile, t);
        const int scan = std::min(SL, std::max(((hi_tile + 1) * ROW_TILE + 1023) / 1024 * 1024, rows_cap));
        hipGraphExec_t exec = nullptr;
        MNXCHK(get_tick_graph(h, scan, rows_cap, nullptr, 0, s, &exec, nullptr, guided));
        for (int i = 0; i < ticks_per_poll; ++i)
            HIPCHK(h, exec ? hipGraphLaunch(exec, s) : enqueue_tick(h, scan, rows_cap, nullptr, 0, s, nullptr, guided));
        HIPCHK(h, dec_enqueue_status(h->db, scan, s));
        int* snap = pinned + (seq & 1) * (1 + MAX_CHUNKS);
        HIPCHK(h, hipMemcpyAsync(snap, &h->db.st->n_active, (size_t)(1 + MAX_CHUNKS) * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipEventRecord(h->ev_poll[seq & 1], s));
        // ---- retire chunks that the PREVIOUS snapshot shows finished (the GPU keeps ticking meanwhile)
        if (seq > 0) {
            const int ps = seq - 1;
            const double tw0 = tf ? now_ms() : 0.0;
            HIPCHK(h, hipEventSynchronize(h->ev_poll[ps & 1]));
            if (tf) host_wait_ms += now_ms() - tw0;
            const int* sn = pinned + (ps & 1) * (1 + MAX_CHUNKS);
            {   // alive rows now <= alive rows in that snapshot + rows admitted after it was taken
                int after = 0;
                for (auto& a : admits) if (a.first > ps) after += a.second;
                bound = std::min(bound, sn[0] + after);
                while (!admits.empty() && admits.front().first <= ps) admits.erase(admits.begin());
            }
            for (size_t i = 0; i < live.size();) {
                Chunk& ck = live[i];
                if (ck.admit_seq <= ps && sn[1 + ck.tag] == 0) {
                    // outputs tile by tile (the bond head's scratch holds 32 rows): rows 32 j .. of the chunk
                    for (int j = 0; j < (int)ck.tiles.size(); ++j) {
                        const int o = ck.first + j * ROW_TILE, nj = std::min(ROW_TILE, ck.n - j * ROW_TILE);
                        int* sl_dev = h->slot_lists + (size_t)ck.tiles[j] * ROW_TILE;
                        int* o_idx = atom_idx + (size_t)o * kmax;
                        int* o_na = n_atoms + o;
                        float* o_logp = conf && conf->token_logp ? conf->token_logp + (size_t)o * max_len : nullptr;
                        double* o_scores = conf ? conf->edge_scores + (size_t)o * kmax * kmax : nullptr;
                        HIPCHK(h, gather_enqueue(h->db, sl_dev, nj, max_len, tokens + (size_t)o * max_len, lengths + o, o_logp,
                                                 nullptr, s));
                        HIPCHK(h, atoms_enqueue(h->db, h->tc_dev, sl_dev, nj, kmax, o_idx, o_na, s));
                        HIPCHK(h, edges_enqueue(h->dw, h->db, h->db.hidden, sl_dev, o_idx, o_na, nj, kmax, h->db.T,
                                                edges + (size_t)o * kmax * kmax, o_scores, s));
                        if (conf)
                            HIPCHK(h, confidence_enqueue(h->db, h->tc_dev, sl_dev, nj, kmax, o_idx, o_na, o_scores,
                                                         conf->atom_scores + (size_t)o * kmax, conf->overall + o, s));
                    }
                    for (int t : ck.tiles) free_tiles.push_back(t);   // handed out again last-first: tiles of a chunk need
                                                                      // be neither contiguous nor ascending
                    live.erase(live.begin() + i);
                    ++done;
                } else {
                    ++i;
                }
            }
        }
        if (tf) fprintf(tf, "%.3f seq %d live %zu next %d next_enc %d done %d free_tiles %zu scan %d rows_cap %d\n",
                        now_ms() - t_begin, seq, live.size(), next, ring.next_enc, done, free_tiles.size(), scan, rows_cap);
        ++seq;
        if (seq > 200000) { h->err = std::string(name) + ": watchdog (decode did not terminate)"; return MNX_ERR_HIP; }
    }
    HIPCHK(h, hipStreamSynchronize(s));
    if (tf) fprintf(tf, "%.3f end host_wait_ms %.3f\n", now_ms() - t_begin, host_wait_ms);
    return check_encoder_range(h, s);
}

extern "C" {

int mnx_predict(mnx_engine* h, const float* images, int32_t n_img, int32_t ref_batch, int32_t max_len,
                int32_t stop_on_eos, int32_t* tokens, int32_t* lengths, int32_t* n_atoms, int32_t* atom_idx,
                uint8_t* edges, int32_t kmax, void* stream) {
    return predict_impl(h, "mnx_predict", images, MNX_IMG_F32, n_img, ref_batch, max_len, stop_on_eos, tokens, lengths, n_atoms, atom_idx,
                        edges, kmax, nullptr, stream);
}

int mnx_predict_confidence(mnx_engine* h, const float* images, int32_t n_img, int32_t ref_batch, int32_t max_len,
                           int32_t* tokens, int32_t* lengths, int32_t* n_atoms, int32_t* atom_idx, uint8_t* edges,
                           int32_t kmax, float* token_logp, double* edge_scores, double* atom_scores, double* overall_score,
                           void* stream) {
    const ConfOut conf{token_logp, edge_scores, atom_scores, overall_score};
    return predict_impl(h, "mnx_predict_confidence", images, MNX_IMG_F32, n_img, ref_batch, max_len, 1, tokens, lengths, n_atoms,
                        atom_idx, edges, kmax, &conf, stream);
}

int mnx_predict_gray8(mnx_engine* h, const uint8_t* gray, int32_t n_img, int32_t ref_batch, int32_t max_len,
                      int32_t* tokens, int32_t* lengths, int32_t* n_atoms, int32_t* atom_idx, uint8_t* edges, int32_t kmax,
                      float* token_logp, double* edge_scores, double* atom_scores, double* overall_score, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    const int n_conf = !!token_logp + !!edge_scores + !!atom_scores + !!overall_score;
    if (n_conf != 0 && n_conf != 4) {
        h->err = "mnx_predict_gray8: the four confidence pointers must be all NULL or all set";
        return MNX_ERR_INVALID_ARG;
    }
    const ConfOut conf{token_logp, edge_scores, atom_scores, overall_score};
    return predict_impl(h, "mnx_predict_gray8", gray, MNX_IMG_GRAY8, n_img, ref_batch, max_len, 1, tokens, lengths, n_atoms,
                        atom_idx, edges, kmax, n_conf ? &conf : nullptr, stream);
}

int mnx_predict_guided(mnx_engine* h, const void* images, int32_t img_format, int32_t n_img, int32_t ref_batch,
                       int32_t max_len, const int32_t* labels, int32_t L, int32_t* tokens, int32_t* lengths, int32_t* n_atoms,
                       int32_t* atom_idx, uint8_t* edges, int32_t kmax, float* token_logp, double* edge_scores,
                       double* atom_scores, double* overall_score, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    if (!labels || L < 2) { h->err = "mnx_predict_guided: labels is null or L < 2"; return MNX_ERR_INVALID_ARG; }
    if (img_format != MNX_IMG_F32 && img_format != MNX_IMG_GRAY8) {
        h->err = "mnx_predict_guided: img_format must be MNX_IMG_F32 or MNX_IMG_GRAY8";
        return MNX_ERR_INVALID_ARG;
    }
    const int n_conf = !!token_logp + !!edge_scores + !!atom_scores + !!overall_score;
    if (n_conf != 0 && n_conf != 4) {
        h->err = "mnx_predict_guided: the four confidence pointers must be all NULL or all set";
        return MNX_ERR_INVALID_ARG;
    }
    const ConfOut conf{token_logp, edge_scores, atom_scores, overall_score};
    return predict_impl(h, "mnx_predict_guided", images, img_format, n_img, ref_batch, max_len, 1, tokens, lengths, n_atoms,
                        atom_idx, edges, kmax, n_conf ? &conf : nullptr, stream, labels, L);
}

int mnx_gemm_clock(mnx_engine* h, int32_t reset, double* mhz) {
    if (!h || !mhz) return MNX_ERR_INVALID_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, x3_clock_read(mhz, reset != 0));
    return MNX_OK;
}

int mnx_probe_mfma(mnx_engine* h, int32_t ms_target, double* tflops, double* mhz, void* stream) {
    if (!h || !tflops || !mhz || ms_target < 1 || ms_target > 2000) return MNX_ERR_INVALID_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    // 8 MFMAs of 16 cycles per iteration and wave, two waves per SIMD: ~256 cycles per iteration at ~1.9 GHz
    const int iters = (int)((double)ms_target * 1e-3 * 1.9e9 / 256.0);
    HIPCHK(h, mfma_probe(iters, (hipStream_t)stream, tflops, mhz));
    return MNX_OK;
}

int mnx_profile_enable(mnx_engine* h, int32_t enable) {
    if (!h) return MNX_ERR_INVALID_ARG;
    h->profiling = enable != 0;
    h->prof_stride = enable > 1 ? enable : 1;
    h->prof_calls = 0;
    h->prof_groups = 0;
    return MNX_OK;
}

int mnx_profile_read(mnx_engine* h, int32_t kind, double* ms_out, double* work_out, int64_t* launches_out) {
    if (!h) return MNX_ERR_INVALID_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    double ms = 0.0, work = 0.0;
    int64_t n = 0;
    for (size_t i = 0; i < h->ev_used; ++i) {
        if (h->ev_pool[i].kind != kind) continue;
        float t = 0.f;
        HIPCHK(h, hipEventSynchronize(h->ev_pool[i].b));
        HIPCHK(h, hipEventElapsedTime(&t, h->ev_pool[i].a, h->ev_pool[i].b));
        ms += t;
        work += h->ev_pool[i].work;
        ++n;
    }
    if (ms_out) *ms_out = ms;
    if (work_out) *work_out = work;
    if (launches_out) *launches_out = n;
    if (kind < 0) h->ev_used = 0;       // kind < 0: reset the pool (after the per-kind reads)
    return MNX_OK;
}

int mnx_probe_decode_attn(mnx_engine* h, int32_t rows, int32_t t, int32_t iters, double* self_ms, double* cross_ms,
                          void* stream) {
    if (!h || rows < 1 || rows > h->db.slots || t < 0 || t >= h->db.T || iters < 1) return MNX_ERR_INVALID_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    for (auto& e : ev) HIPCHK(h, hipEventCreate(&e));
    hipError_t err = dec_probe_attn(h->dw, h->db, rows, t, iters, ev, s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    float a = 0.f, b = 0.f;
    if (err == hipSuccess) err = hipEventElapsedTime(&a, ev[0], ev[1]);
    if (err == hipSuccess) err = hipEventElapsedTime(&b, ev[2], ev[3]);
    for (auto& e : ev) hipEventDestroy(e);
    if (err != hipSuccess) { h->err = std::string("mnx_probe_decode_attn: ") + hipGetErrorString(err); return MNX_ERR_HIP; }
    if (self_ms) *self_ms = (double)a / iters;
    if (cross_ms) *cross_ms = (double)b / iters;
    return MNX_OK;
}

int mnx_gemm16(mnx_engine* h, int32_t epi, const void* A, const void* W, void* C, const float* bias, int32_t M,
               int32_t N, int32_t K, void* stream) {
    if (!h || !A || !W || !C) return MNX_ERR_INVALID_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    const int dt = dt_base(h->dt);
    if (!bias && N <= h->zero_bias_n) bias = h->zero_bias;
    if (epi & 0x100) {      // test aid: the persistent fp32-output kernel (gemm_res.hip) whatever the dispatch would choose
        epi &= 0xff;
        if (!gemm_res_supports(dt, epi, M, N, K)) { h->err = "mnx_gemm16: shape / epilogue not supported by gemm_res"; return MNX_ERR_INVALID_ARG; }
        HIPCHK(h, launch_gemm_res(dt, epi, A, W, (float*)C, bias, epi == EPI_RESID_F32 ? (const float*)C : nullptr, M, N, K,
                                  (hipStream_t)stream));
        return MNX_OK;
    }
    HIPCHK(h, launch_gemm16(dt, epi, A, W, C, bias, epi == EPI_RESID_F32 ? (const float*)C : nullptr, M, N, K,
                            (hipStream_t)stream));
    return MNX_OK;
}

int mnx_gemm16_split(mnx_engine* h, int32_t epi, const void* A, int64_t a_lo, const void* W, int64_t w_lo, float oscale,
                     void* C, int64_t c_lo, const float* bias, int32_t M, int32_t N, int32_t K, int32_t terms,
                     void* stream) {
    if (!h || !A || !W || !C) return MNX_ERR_INVALID_ARG;
    if (!dt_split(h->dt)) { h->err = "mnx_gemm16_split: the engine's compute_dtype is not a split mode"; return MNX_ERR_INVALID_ARG; }
    if (a_lo < 0 || w_lo < 0 || c_lo < 0) { h->err = "mnx_gemm16_split: negative plane offset"; return MNX_ERR_INVALID_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    if (!bias) {            // the kernels take a bias vector unconditionally: the engine's zero vector stands in
        if (N > h->zero_bias_n) { h->err = "mnx_gemm16_split: bias == NULL needs N <= 2 * the widest stage"; return MNX_ERR_CAPACITY; }
        bias = h->zero_bias;
    }
    if (terms < 1 || terms > 3 || (terms == 2 && h->dt != MNX_DT_F16X3)) {
        h->err = "mnx_gemm16_split: terms must be 1, 3 or (FP16X3 / FP16X3M only) 2";
        return MNX_ERR_INVALID_ARG;
    }
    SplitArgs sp;
    sp.a_lo = (size_t)a_lo; sp.w_lo = (size_t)w_lo; sp.c_lo = (size_t)c_lo; sp.oscale = oscale; sp.terms = terms;
    if (epi & 0x400) { sp.c_planes = 1; epi &= ~0x400; }      // 16-bit epilogues: the hi output plane only
    if (epi & 0x200) {      // test aid: the 128x128 kernel whatever the dispatch would choose
        epi &= 0xff;
        HIPCHK(h, launch_gemm16_tile128(h->dt, epi, A, W, C, bias, epi == EPI_RESID_F32 ? (const float*)C : nullptr, M, N, K,
                                        (hipStream_t)stream, &sp));
        return MNX_OK;
    }
    if (epi & 0x100) {      // test aid: gemm_res.hip whatever the dispatch would choose
        epi &= 0xff;
        if (!gemm_res_supports(h->dt, epi, M, N, K)) { h->err = "mnx_gemm16_split: not supported by gemm_res"; return MNX_ERR_INVALID_ARG; }
        HIPCHK(h, launch_gemm_res(h->dt, epi, A, W, (float*)C, bias, epi == EPI_RESID_F32 ? (const float*)C : nullptr,
                                  M, N, K, (hipStream_t)stream, &sp));
        return MNX_OK;
    }
    HIPCHK(h, launch_gemm16(h->dt, epi, A, W, C, bias, epi == EPI_RESID_F32 ? (const float*)C : nullptr, M, N,
                            K, (hipStream_t)stream, &sp));
    return MNX_OK;
}

int mnx_window_attn(mnx_engine* h, const void* qkv, int64_t qkv_lo, const float* table, void* out, int64_t out_lo,
                    int32_t B, int32_t H, int32_t W, int32_t C, int32_t heads, int32_t shift, int32_t terms, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const char* m) { h->err = std::string("mnx_window_attn: ") + m; return MNX_ERR_INVALID_ARG; };
    if (!qkv || !table || !out) return bad("null pointer");
    if (((uintptr_t)qkv | (uintptr_t)out) & 15) return bad("qkv and out must be 16-byte aligned");
    if (B < 1 || H < 12 || W < 12 || H % 12 || W % 12) return bad("B >= 1 and H, W positive multiples of the window (12) required");
    if (heads < 1 || C != heads * 32) return bad("C must be heads * 32 (head_dim 32)");
    if (shift < 0 || shift >= 12) return bad("shift must be 0..11");
    const int64_t rows = (int64_t)B * H * W;
    if (rows > INT32_MAX || (int64_t)B * (H / 12) * (W / 12) * heads > INT32_MAX)
        return bad("B * H * W and the number of (window, head) items must fit in int32");
    const bool split = dt_split(h->dt);
    const int base = terms & 0xff;
    if ((terms & ~0x1ff) || (split ? (base != 1 && base != 3) || ((terms & 0x100) && base != 3) : terms != 1))
        return bad("terms must be 1 or 3 (| 0x100 with 3) for the split compute_dtypes and 1 for the others");
    if (split) {
        if (qkv_lo < rows * 3 * C || out_lo < rows * C || (qkv_lo | out_lo) & 7)
            return bad("qkv_lo / out_lo must be at least the hi plane's size and multiples of 8 elements");
        if ((int64_t)H * W * 3 * C * 2 > ((int64_t)1 << 32)) return bad("one image's qkv plane exceeds 2^32 bytes");
    } else if (qkv_lo || out_lo) {
        return bad("qkv_lo / out_lo must be 0 for the single-plane compute_dtypes");
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, launch_window_attn(h->dt, qkv, table, out, B, H, W, C, heads, shift, (hipStream_t)stream, (size_t)qkv_lo,
                                 (size_t)out_lo, terms));
    return MNX_OK;
}

int mnx_kv_block(mnx_engine* h, int32_t which, int32_t layer, int32_t owner, int32_t head, void* dst, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const char* m) { h->err = std::string("mnx_kv_block: ") + m; return MNX_ERR_INVALID_ARG; };
    const mnx_config& c = h->cfg;
    const DecBuffers& db = h->db;
    if (!dst) return bad("null dst");
    if (which < 0 || which > 3) return bad("which must be 0 (self K), 1 (self V), 2 (memory K) or 3 (memory V)");
    if (layer < 0 || layer >= c.dec_layers || head < 0 || head >= c.dec_heads) return bad("layer or head out of range");
    const char* src;
    size_t bytes;
    if (which < 2) {
        if (owner < 0 || owner >= db.slots) return bad("slot out of range");
        bytes = kvq_block_bytes(db.Tq);   // self_k / self_v: [layer][slot][head] blocks of Tq rows
        src = (which == 0 ? db.self_k : db.self_v) + (((size_t)layer * db.slots + owner) * c.dec_heads + head) * bytes;
    } else {
        if (owner < 0 || owner >= db.mem_blocks) return bad("memory block out of range");
        bytes = kvq_block_bytes(db.Sq);   // mem_kv: [memory block][layer][K|V][head] blocks of Sq rows
        src = db.mem_kv + ((((size_t)owner * c.dec_layers + layer) * 2 + (which - 2)) * c.dec_heads + head) * bytes;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MNX_OK;
}

int mnx_beam_scripted(mnx_engine* h, const float* table, int32_t B, int32_t beam, int32_t n_best, int32_t max_len, int32_t V,
                      int32_t eos, int32_t* tokens, int32_t* lengths, float* scores, int32_t* steps_run, int32_t* tr_parent,
                      int32_t* tr_token, float* tr_score, int32_t* tr_alive, int32_t* tr_n_active, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const char* m) { h->err = std::string("mnx_beam_scripted: ") + m; return MNX_ERR_INVALID_ARG; };
    const mnx_config& c = h->cfg;
    if (!table || !tokens || !lengths || !scores || !steps_run) return bad("null table, tokens, lengths, scores or steps_run");
    const int n_tr = !!tr_parent + !!tr_token + !!tr_score + !!tr_alive + !!tr_n_active;
    if (n_tr != 0 && n_tr != 5) return bad("the five trace pointers must be all null or all set");
    if (B < 1) return bad("B must be 1..32");
    if (beam < 1 || beam > MAX_BEAM) return bad("beam must be 1..8");
    if (n_best < 1 || n_best > beam) return bad("n_best must be 1..beam");
    if (V < 2 || V > BEAM_LP_STRIDE) return bad("V must be 2..256");
    if (eos < 0 || eos >= V) return bad("eos must be 0..V-1");
    if (max_len < 1 || max_len > c.max_len || c.max_len + 1 > BEAM_ANC_MAX) return bad("max_len must be 1..cfg.max_len (<= 511)");
    // the pool first: with B <= 32 it keeps 8 per image, so only a larger B can ask for more than it holds
    if (n_best > beam_pool_stride(B)) return bad("n_best exceeds the hypotheses the pool keeps per image (256 / B)");
    if (B > ROW_TILE) return bad("B must be 1..32");
    if (B * beam > h->db.slots) return bad("B x beam exceeds dec_slots");
    hipStream_t s;
    MNXCHK(caller_stream(h, stream, &s));
    MNXCHK(beam_buffers(h, B, B, beam, n_best, false));
    MNXCHK(lazy_alloc(h, &h->script_nact, (size_t)c.max_len * 4));
    BeamBuffers run = h->beam;
    run.phid = nullptr;
    run.tr_parent = tr_parent; run.tr_token = tr_token; run.tr_score = tr_score; run.tr_alive = tr_alive;
    HIPCHK(h, dec_enqueue_reset(h->db, s));
    HIPCHK(h, beam_enqueue_init(h->db, run, max_len, s));
    const int rows = (B * beam + ROW_TILE - 1) / ROW_TILE * ROW_TILE;
    int step = 0;       // steps enqueued so far; the loop is run_steps' (groups of 8, then the alive count), without a graph
    MNXCHK(run_steps(h, nullptr, [&]() { return beam_enqueue_script_step(h->db, run, table, V, eos, h->script_nact + step++, s); },
                     rows, max_len, s));
    HIPCHK(h, beam_enqueue_gather(h->db, run, max_len, tokens, lengths, scores, nullptr, s));
    std::vector<int> nact(step);
    HIPCHK(h, hipMemcpyAsync(nact.data(), h->script_nact, (size_t)step * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    int n_run = 0;      // a step whose begin kernel found no row alive ran nothing
    while (n_run < step && nact[n_run] > 0) ++n_run;
    if (tr_n_active && n_run)
        HIPCHK(h, hipMemcpyAsync(tr_n_active, h->script_nact, (size_t)n_run * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));
    *steps_run = n_run;
    return MNX_OK;
}

int mnx_decode_beam_forced(mnx_engine* h, const float* features, int32_t B, int32_t beam, int32_t n_best, int32_t max_len,
                           const int32_t* script_parent, const int32_t* script_token, int64_t script_len, int32_t* tokens,
                           int32_t* lengths, float* scores, float* hidden, float* logits_trace, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const std::string& m) { h->err = "mnx_decode_beam_forced: " + m; return MNX_ERR_INVALID_ARG; };
    const mnx_config& c = h->cfg;
    if (!features || !script_parent || !script_token || !tokens || !lengths || !scores)
        return bad("null features, script_parent, script_token, tokens, lengths or scores");
    if (B < 1 || B > ROW_TILE) return bad("B must be 1..32");
    if (beam < 1 || beam > MAX_BEAM) return bad("beam must be 1..8");
    if (n_best < 1 || n_best > beam) return bad("n_best must be 1..beam");
    if (max_len < 1 || max_len > c.max_len || c.max_len + 1 > BEAM_ANC_MAX) return bad("max_len must be 1..cfg.max_len (<= 511)");
    if (c.vocab > BEAM_LP_STRIDE) return bad("the vocabulary exceeds 256 ids");
    if (B * beam > h->db.slots) return bad("B x beam exceeds dec_slots");
    const size_t n = (size_t)max_len * B * beam;
    if (script_len < 0 || (uint64_t)script_len < n) return bad("script_len is less than max_len x B x beam");
    // the script as the device will read it: every element checked on its way into the copy that is uploaded
    std::vector<int> script(2 * n);
    auto at = [&](size_t i, int x) {
        return "[" + std::to_string(i / ((size_t)B * beam)) + "][" + std::to_string(i / beam % B) + "][" + std::to_string(i % beam) +
               "] = " + std::to_string(x);
    };
    for (size_t i = 0; i < n; ++i) {
        const int p = script_parent[i], v = script_token[i];
        if (p < 0 || p >= beam) return bad("script_parent" + at(i, p) + " is outside 0..beam-1");
        if (v < 0 || v >= c.vocab) return bad("script_token" + at(i, v) + " is outside 0..vocab-1");
        script[i] = p; script[n + i] = v;
    }
    hipStream_t s;
    MNXCHK(caller_stream(h, stream, &s));
    MNXCHK(lazy_alloc(h, &h->beam_script, (size_t)2 * c.max_len * ROW_TILE * MAX_BEAM * 4));
    HIPCHK(h, hipMemcpyAsync(h->beam_script, script.data(), 2 * n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));      // `script` is pageable host memory of this call
    return decode_beam_groups(h, &features, 1, B, B, beam, n_best, max_len, tokens, lengths, scores, hidden, s, h->beam_script,
                              logits_trace);
}

// ---- test aids: the encoder's non-GEMM kernels and the fp32 SGEMM on caller buffers (tests/test_gpu_encoder_ops.py) ----
// Each checks everything its launcher assumes (and what the launcher leaves to the encoder: positive sizes, alignment of
// the 16-byte accesses) and launches nothing when it refuses.
static bool misaligned16(std::initializer_list<const void*> ps) {
    uintptr_t a = 0;
    for (const void* p : ps) a |= (uintptr_t)p;
    return (a & 15) != 0;
}

int mnx_patch_embed(mnx_engine* h, const void* img, int32_t img_format, const float* w_t, const float* bias,
                    const float* gamma, const float* beta, float* x, int32_t B, int32_t S, int32_t C, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const char* m) { h->err = std::string("mnx_patch_embed: ") + m; return MNX_ERR_INVALID_ARG; };
    if (img_format != MNX_IMG_F32 && img_format != MNX_IMG_GRAY8) return bad("img_format must be MNX_IMG_F32 or MNX_IMG_GRAY8");
    if (!img || !w_t || !bias || !gamma || !beta || !x) return bad("null pointer");
    if (misaligned16({w_t, bias, gamma, beta, x})) return bad("w_t, bias, gamma, beta and x must be 16-byte aligned");
    if ((uintptr_t)img & (img_format == MNX_IMG_GRAY8 ? 3 : 15))
        return bad("img must be 16-byte (MNX_IMG_F32) or 4-byte (MNX_IMG_GRAY8) aligned");
    if (C < 32 || C > 128 || (C & 31)) return bad("C must be 32, 64, 96 or 128");
    if (S < 4 || (S & 3)) return bad("S must be a positive multiple of the patch size (4)");
    if (B < 1 || B > 65535) return bad("B must be 1..65535");
    if ((int64_t)B * (S / 4) * (S / 4) > INT32_MAX) return bad("B * (S/4)^2 must fit in int32");
    HIPCHK(h, hipSetDevice(h->device));
    if (img_format == MNX_IMG_GRAY8)
        HIPCHK(h, launch_patch_embed_gray8((const uint8_t*)img, w_t, bias, gamma, beta, x, B, S, C, (hipStream_t)stream));
    else
        HIPCHK(h, launch_patch_embed((const float*)img, w_t, bias, gamma, beta, x, B, S, C, (hipStream_t)stream));
    return MNX_OK;
}

int mnx_layernorm16(mnx_engine* h, const float* x, const float* gamma, const float* beta, void* y16, int64_t y_lo,
                    float* y32, int32_t M, int32_t C, float eps, int32_t planes, int32_t* flag, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const char* m) { h->err = std::string("mnx_layernorm16: ") + m; return MNX_ERR_INVALID_ARG; };
    if (!x || !gamma || !beta) return bad("null pointer");
    if (!y16 && !y32) return bad("y16 and y32 are both null");
    if (misaligned16({x, gamma, beta, y32}) || ((uintptr_t)y16 & 7) || (h->dt == MNX_DT_F32 && ((uintptr_t)y16 & 15)))
        return bad("x, gamma, beta and y32 must be 16-byte aligned, y16 8-byte (16-byte for FP32)");
    if ((uintptr_t)flag & 3) return bad("flag must be 4-byte aligned");
    if (M < 1 || (int64_t)M + 8 > INT32_MAX) return bad("M must be positive (and M + 8 fit in int32)");
    if (C < 4 || C > 2048 || (C & 3)) return bad("C must be a multiple of 4 in 4..2048");
    if (!(eps >= 0.f)) return bad("eps must be >= 0");
    if (planes != 1 && planes != 2) return bad("planes must be 1 or 2");
    if (dt_split(h->dt)) {
        if (planes == 2 && y16 && (y_lo < (int64_t)M * C || (y_lo & 7)))
            return bad("y_lo must be at least M * C and a multiple of 8 elements");
        if (y_lo < 0) return bad("y_lo must not be negative");
    } else if (y_lo || planes != 2) {
        return bad("y_lo must be 0 and planes 2 for the single-plane compute_dtypes");
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, launch_layernorm16(h->dt, x, gamma, beta, y16, y32, M, C, eps, (hipStream_t)stream, (size_t)y_lo, flag, planes));
    return MNX_OK;
}

int mnx_merge_ln16(mnx_engine* h, const float* x, const float* gamma, const float* beta, void* y16, int64_t y_lo,
                   int32_t B, int32_t H, int32_t W, int32_t C, float eps, int32_t planes, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const char* m) { h->err = std::string("mnx_merge_ln16: ") + m; return MNX_ERR_INVALID_ARG; };
    if (!x || !gamma || !beta || !y16) return bad("null pointer");
    if (misaligned16({x, gamma, beta}) || ((uintptr_t)y16 & 7) || (h->dt == MNX_DT_F32 && ((uintptr_t)y16 & 15)))
        return bad("x, gamma and beta must be 16-byte aligned, y16 8-byte (16-byte for FP32)");
    if (B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1)) return bad("B >= 1 and H, W positive even numbers required");
    if (C < 4 || 4 * (int64_t)C > 2048 || (C & 3)) return bad("C must be a multiple of 4 in 4..512");
    if ((int64_t)B * H * W > INT32_MAX) return bad("B * H * W must fit in int32");
    if (!(eps >= 0.f)) return bad("eps must be >= 0");
    if (planes != 1 && planes != 2) return bad("planes must be 1 or 2");
    const int64_t out = (int64_t)B * (H / 2) * (W / 2) * 4 * C;
    if (dt_split(h->dt)) {
        if (planes == 2 && (y_lo < out || (y_lo & 7))) return bad("y_lo must be at least B * H/2 * W/2 * 4C and a multiple of 8 elements");
        if (y_lo < 0) return bad("y_lo must not be negative");
    } else if (y_lo || planes != 2) {
        return bad("y_lo must be 0 and planes 2 for the single-plane compute_dtypes");
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, launch_merge_ln16(h->dt, x, gamma, beta, y16, B, H, W, C, eps, (hipStream_t)stream, (size_t)y_lo, planes));
    return MNX_OK;
}

int mnx_cast16(mnx_engine* h, const float* x, void* y16, int64_t y_lo, int64_t n, float scale, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const char* m) { h->err = std::string("mnx_cast16: ") + m; return MNX_ERR_INVALID_ARG; };
    if (!x || !y16) return bad("null pointer");
    if (((uintptr_t)x & 15) || ((uintptr_t)y16 & 7) || (h->dt == MNX_DT_F32 && ((uintptr_t)y16 & 15)))
        return bad("x must be 16-byte aligned, y16 8-byte (16-byte for FP32)");
    if (n < 4 || (n & 3)) return bad("n must be a positive multiple of 4");
    if (dt_split(h->dt)) {
        if (y_lo < n || (y_lo & 3)) return bad("y_lo must be at least n and a multiple of 4 elements");
        if (!(scale > 0.f) || !(scale < INFINITY)) return bad("scale must be positive and finite");
    } else if (y_lo) {
        return bad("y_lo must be 0 for the single-plane compute_dtypes");
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, launch_cast16(h->dt, x, y16, (size_t)n, (hipStream_t)stream, (size_t)y_lo, scale));
    return MNX_OK;
}

int mnx_sgemm_tn(mnx_engine* h, const float* A, const float* W, const float* bias, float* C, int32_t M, int32_t N,
                 int32_t K, int32_t perm_S, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const char* m) { h->err = std::string("mnx_sgemm_tn: ") + m; return MNX_ERR_INVALID_ARG; };
    if (!A || !W || !C) return bad("null pointer");
    if (misaligned16({A, W, bias, C})) return bad("A, W, bias and C must be 16-byte aligned");
    if (M < 1 || N < 4 || K < 16) return bad("M >= 1, N >= 4 and K >= 16 required");
    if (K & 15) return bad("K must be a multiple of 16");
    if (N & 3) return bad("N must be a multiple of 4");
    if (perm_S < 0) return bad("perm_S must not be negative");
    if (perm_S > 0 && (N & 255)) return bad("perm_S needs N to be a multiple of 256");
    if (perm_S > 0 && M % perm_S) return bad("perm_S must divide M");
    if ((M + 63) / 64 > 65535) return bad("M must be at most 65535 * 64");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, launch_sgemm_tn(A, W, bias, C, M, N, K, (hipStream_t)stream, perm_S));
    return MNX_OK;
}

}  // extern "C"
