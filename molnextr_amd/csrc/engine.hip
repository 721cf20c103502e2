// engine.hip — host side of libmolnextr_hip.so, the model path: weight packing, workspace, encode/decode/edges orchestration,
// hipGraph replay of the decode step. Implements the model's part of include/molnextr_hip.h; the packed-table entry points are
// engine_tables.hip, the test aids and probes engine_lab.hip, what the three share engine_impl.h.
#include <time.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <unordered_map>

#include "engine_impl.h"
#include "kernels.h"
#include "kvq.h"

using namespace mnx;

#ifndef MNX_PLANE_SKEW
#define MNX_PLANE_SKEW 4352
#endif
static constexpr size_t PLANE_SKEW = MNX_PLANE_SKEW;   // elements (8704 bytes; 16-byte aligned for the LDS-DMA)

namespace {

thread_local std::string g_create_error;   // message of the calling thread's last failed mnx_create

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

namespace mnx {

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

}  // namespace mnx

namespace {

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

}  // namespace

namespace mnx {

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
                       const int* script, float* logits_trace) {
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

}  // namespace mnx

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

}  // extern "C"
