// engine_lab.hip — host side of libmolnextr_hip.so, the test aids and probes of include/molnextr_hip.h: single kernels on caller
// buffers, scripted beam searches, the clocks and profiles of the benchmark tools. Nothing here is on the predict path.
#include <cmath>
#include <cstring>

#include "engine_impl.h"
#include "kernels.h"
#include "kvq.h"

using namespace mnx;

extern "C" {

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

// What the GEMM test aids refuse before any launch, in words (the launchers repeat the shape checks, but their refusal is a
// bare hipErrorInvalidValue, and a null pointer used to return without touching the handle's error text at all).
static const char* gemm16_refusal(int dtype, const void* A, const void* W, const void* C, int M, int N, int K) {
    if (!A || !W || !C) return "null A, W or C";
    if (M <= 0) return "M must be positive";
    if (K <= 0 || (K & 7) || N <= 0 || (N & 7)) return "K and N must be positive multiples of 8";
    if (dt_base(dtype) == MNX_DT_F32 && (K & 15)) return "the fp32 kernel needs K to be a multiple of 16";
    return nullptr;
}

int mnx_gemm16(mnx_engine* h, int32_t epi, const void* A, const void* W, void* C, const float* bias, int32_t M,
               int32_t N, int32_t K, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    if (const char* why = gemm16_refusal(h->dt, A, W, C, M, N, K)) { h->err = std::string("mnx_gemm16: ") + why; return MNX_ERR_INVALID_ARG; }
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
    if (!h) return MNX_ERR_INVALID_ARG;
    if (const char* why = gemm16_refusal(h->dt, A, W, C, M, N, K)) { h->err = std::string("mnx_gemm16_split: ") + why; return MNX_ERR_INVALID_ARG; }
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

// ---- test aid: one linear of the 8-launches-per-layer decode tick on caller buffers (tests/test_gpu_dec_linear.py) ----
int mnx_dec_linear(mnx_engine* h, int32_t pro, int32_t epi, const float* in, const float* W, const float* bias,
                   const float* gamma, const float* beta, const float* part, int32_t n_part, int32_t part_stride, float* out,
                   float* x_write, int32_t N, int32_t K, int32_t capacity, int32_t n_alive, const int32_t* rows, void* stream) {
    if (!h) return MNX_ERR_INVALID_ARG;
    auto bad = [&](const std::string& m) { h->err = "mnx_dec_linear: " + m; return MNX_ERR_INVALID_ARG; };
    const mnx_config& c = h->cfg;
    const DecBuffers& db = h->db;
    if (!dec_linear_instantiated(pro, epi))
        return bad("(pro, epi) must be one of the instantiated pairs (2,0), (1,0), (0,1), (1,2), (1,3), (0,4)");
    const bool reads_part = pro == 1 && part;
    if (!W || !bias || !out || !rows || (pro != 2 && !in) || (pro != 0 && (!gamma || !beta)) || ((pro == 2 || reads_part) && !x_write))
        return bad("null pointer (W, bias, out, rows; in unless pro = 2; gamma, beta unless pro = 0; x_write with pro = 2 or part)");
    if (part && pro != 1) return bad("part is read by pro = 1 alone and must be null otherwise");
    if (misaligned16({in, W, bias, gamma, beta, part, out, x_write}))
        return bad("in, W, bias, gamma, beta, part, out and x_write must be 16-byte aligned");
    if (capacity < ROW_TILE || capacity % ROW_TILE || capacity > db.slots)
        return bad("capacity must be a multiple of 32 in 32..dec_slots");
    if (n_alive < 1 || n_alive > capacity || n_alive > c.pe_len) return bad("n_alive must be 1..capacity (and at most pe_len)");
    if (N < 32 || N % 32 || N > 65536) return bad("N must be a multiple of 32 in 32..65536");
    if (K < 256 || K % 256 || K > 16384) return bad("K must be a multiple of 256 in 256..16384");
    if (pro != 0 && K != 256) return bad("K must be 256 with pro = 1 or 2 (the LayerNorm row)");
    if (epi == 0 && N != 768) return bad("N must be 768 with epi = 0 (query | keys | values)");
    if (epi == 0 && (c.dec_dim != 256 || c.dec_heads != 8)) return bad("epi = 0 needs an engine of dec_dim 256 and 8 heads");
    if (reads_part && (n_part < 1 || n_part > 16)) return bad("n_part must be 1..16 with part");
    if ((reads_part || epi == 4) && (part_stride % 4 || (int64_t)part_stride < (int64_t)capacity * (epi == 4 ? N : 256)))
        return bad("part_stride must be a multiple of 4 and at least capacity * 256 (epi = 4: capacity * N) floats");
    if (epi == 4 && (int64_t)part_stride * (K / 256) > INT32_MAX) return bad("part_stride * K / 256 must fit in int32");
    std::vector<int> script((size_t)n_alive * 4);
    std::vector<char> seen((size_t)db.slots, 0);
    for (int i = 0; i < n_alive; ++i) {
        const int slot = rows[4 * i], t = rows[4 * i + 1], tok = rows[4 * i + 2], rowc = rows[4 * i + 3];
        const std::string at = "rows[" + std::to_string(i) + "]: ";
        if (slot < 0 || slot >= db.slots) return bad(at + "slot " + std::to_string(slot) + " is outside 0..dec_slots-1");
        if (seen[slot]) return bad(at + "slot " + std::to_string(slot) + " is repeated");
        seen[slot] = 1;
        if (t < 0 || t >= c.max_len) return bad(at + "t " + std::to_string(t) + " is outside 0..max_len-1");
        if (tok < 0 || tok >= c.vocab) return bad(at + "prev_tok " + std::to_string(tok) + " is outside 0..vocab-1");
        if (rowc < 0 || rowc >= MAX_REF_BATCH) return bad(at + "rowc " + std::to_string(rowc) + " is outside 0..511");
        for (int j = 0; j < 4; ++j) script[4 * i + j] = rows[4 * i + j];
    }
    hipStream_t s;
    MNXCHK(caller_stream(h, stream, &s));
    MNXCHK(lazy_alloc(h, &h->lin_script, (size_t)MAX_SLOTS * 4 * sizeof(int)));
    HIPCHK(h, hipMemcpyAsync(h->lin_script, script.data(), script.size() * sizeof(int), hipMemcpyHostToDevice, s));
    DecLinearCall call = {};
    call.pro = pro; call.epi = epi; call.in = in; call.W = W; call.bias = bias; call.gamma = gamma; call.beta = beta;
    call.part = reads_part ? part : nullptr; call.n_part = n_part; call.part_stride = part_stride; call.out = out;
    call.x_write = x_write; call.N = N; call.K = K; call.capacity = capacity; call.n_alive = n_alive;
    call.rows = (const int4*)h->lin_script;
    HIPCHK(h, dec_lab_linear(h->dw, h->db, call, s));
    HIPCHK(h, hipStreamSynchronize(s));      // `script` is pageable host memory of this call
    return MNX_OK;
}

}  // extern "C"
