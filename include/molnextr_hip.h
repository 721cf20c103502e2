/* molnextr_hip.h — C ABI of libmolnextr_hip.so, the MI355X (gfx950) engine behind the MolNexTR predict path.
 *
 * The reference (CYF2000127/MolNexTR) has no plugin / FFI interface; the seam this library sits behind is the
 * pair of Python calls in `molnextr.predict_images`
 *
 *     features, hiddens = self.encoder(images)                      MolNexTR/model.py:107   (main.py:279)
 *     batch_predictions = self.decoder.decode(features, hiddens)    MolNexTR/model.py:108   (main.py:280)
 *
 * Each entry point below names the reference code it replaces. All functions are `extern "C"`, take plain
 * pointers and sizes (no torch / C++ types), return 0 on success or a negative mnx_status, never throw, and
 * enqueue their GPU work on the caller's HIP stream. Device pointers are raw HBM addresses (e.g. a PyTorch-ROCm
 * tensor's data_ptr()). A handle is bound to one device and is not re-entrant: one in-flight call per handle —
 * except that ONE call of the preprocess family (mnx_preprocess or mnx_preprocess_batch; their only state is private box
 * scratch) may run on another thread and stream beside any other entry point, so that the next pages can be uploaded and
 * transformed while mnx_predict works; different handles (GPUs) may be driven from different threads or processes. The only process-wide state is the
 * message of the last failed mnx_create (read it with mnx_last_error(NULL) from the thread that called mnx_create).
 */
#ifndef MOLNEXTR_HIP_H
#define MOLNEXTR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MNX_ABI_VERSION 7

typedef struct mnx_engine mnx_engine;

typedef enum {
    MNX_OK = 0,
    MNX_ERR_INVALID_ARG = -1,   /* bad pointer / size / config                                   */
    MNX_ERR_WEIGHTS = -2,       /* a tensor of the weight contract is missing or has a wrong shape */
    MNX_ERR_HIP = -3,           /* a HIP runtime call failed (see mnx_last_error)                 */
    MNX_ERR_NO_DEVICE = -4,     /* no gfx950 device at the requested index                        */
    MNX_ERR_CAPACITY = -5,      /* batch / length / atom count exceeds what mnx_create reserved   */
    MNX_ERR_RANGE = -6          /* the encoder produced non-finite features (fp16 operand range)  */
} mnx_status;

/* Operand type of the encoder MFMA GEMMs / window attention (accumulation, residual stream, LayerNorm and softmax are
 * fp32 in every mode; the decoder and the bond head are fp32 always).
 *   BF16, FP16     one 16-bit plane per operand: the fastest modes; the operand rounding (2^-9 / 2^-12 relative) reaches
 *                  the logits as 6e-2 / 9e-3, so argmax decisions near a tie can differ from the reference;
 *   FP16X3, BF16X3 split operands: every GEMM / attention operand v is carried as two 16-bit planes hi = T(v),
 *                  lo = T(v - hi), every product evaluated as hi.hi + hi.lo + lo.hi on the 16-bit MFMA with fp32
 *                  accumulation, exact-erf GELU. FP16X3 (weights stored scaled by a power of two per matrix so that their
 *                  lo planes are normal numbers) reproduces the fp32 path to fp32 rounding level: tokens / atoms / bonds
 *                  equal the reference from pixels at a third of the 16-bit MFMA rate. This is the default of the Python
 *                  facade and of bench.py. Activations must stay inside the fp16 range (|v| < 65504): a non-finite
 *                  encoder output is reported as MNX_ERR_RANGE by mnx_predict / mnx_predict_beam and by
 *                  mnx_encoder_status; BF16X3 has the fp32 range and ~2^-16 relative product error;
 *   FP32           every encoder operand in fp32 on the exact-fp32 matrix instructions (1/16 of the bf16 rate): the
 *                  reference-arithmetic mode the split modes are checked against;
 *   FP16X3M        FP16X3 with a per-stage, per-op-class term count ("M" = mixed): the op classes of
 *                  MNX_FP16X3M_TWO_TERM_BY_STAGE evaluate
 *                  a.w as ah.wh + ah.wl — the ACTIVATION's lo plane is neither written by its producer nor read nor
 *                  multiplied; the weight keeps both planes (its rounding is systematic over every token, the
 *                  activation's is noise: dropping ah.wl instead costs 3x the error). Two thirds of the matrix work and half
 *                  the activation bytes in those layers (60 % of the encoder's GEMM time: qkv, fc1, fc2 of Swin stage 3).
 *                  Measured from pixels on both fixture checkpoints: every token / atom / bond still equal to the
 *                  reference's, 0 argmax flips in 12863 teacher-forced steps, log-probs within 1.8e-4, raw logits within
 *                  5.0e-4 (FP16X3: 2e-5 / 8e-5; north_star allows 1e-3); on 384 further images against the oracle the raw
 *                  logits reach 8.7e-4, on 384 more of a hostile checkpoint 1.2e-3 (FP16X3: 2.4e-4), still 0 flips in 220 000
 *                  steps — an OPT-IN throughput mode for callers who accept logits at north_star's edge: the
 *                  default stays FP16X3 (profiles/r06_two_term_tables_gpu.json, r06_extended_parity_*.json, DESIGN.md
 *                  section 4.3, tests/test_gpu_pixels.py).
 *                  Same weights, range and MNX_ERR_RANGE behaviour as FP16X3. mnx_set_op_terms changes the table. */
enum { MNX_DTYPE_BF16 = 0, MNX_DTYPE_FP16 = 1, MNX_DTYPE_FP32 = 2, MNX_DTYPE_BF16X3 = 3, MNX_DTYPE_FP16X3 = 4,
       MNX_DTYPE_FP16X3M = 5 };
/* op classes of the split modes (bits of mnx_set_split_terms / mnx_set_op_terms) */
enum { MNX_OP_QKV = 1, MNX_OP_ATTN = 2, MNX_OP_PROJ = 4, MNX_OP_FC1 = 8, MNX_OP_FC2 = 16, MNX_OP_MERGE = 32 };
/* FP16X3M's table: the two-term op classes of Swin-B's stages 1..4 (the patch-merging reduction BEHIND stage s counts as
 * stage s). tools/study_split_terms.py --two is the CPU emulation that picked it, tests/test_gpu_pixels.py the gate. */
#define MNX_FP16X3M_TWO_TERM_BY_STAGE { 0, 0, MNX_OP_QKV | MNX_OP_FC1 | MNX_OP_FC2, 0 }
#define MNX_FP16X3M_FIRST_BLOCK_BY_STAGE { 0, 0, 0, 0 }     /* first Swin block of the stage that runs the table (all: 0) */

/* Architecture + capacity. Defaults of the reference inference config are in the comments
 * (MolNexTR/models/transformers.py:547-551 swin_base; MolNexTR/model.py:50-81; MolNexTR/utils.py:25). */
typedef struct {
    int32_t img_size;        /* 384; every stage's grid a multiple of `window`, the last stage's grid <= 512 positions */
    int32_t patch;           /* 4   */
    int32_t embed_dim;       /* 128 */
    int32_t n_stages;        /* 4   */
    int32_t depths[4];       /* 2,2,18,2   */
    int32_t heads[4];        /* 4,8,16,32  (head_dim must be 32) */
    int32_t window;          /* 12 */
    int32_t dec_layers;      /* 6   */
    int32_t dec_dim;         /* 256 */
    int32_t dec_heads;       /* 8   */
    int32_t dec_ff;          /* 1024 */
    int32_t vocab;           /* 229 = 101 symbols + 64 x-bins + 64 y-bins */
    int32_t sym_offset;      /* 101: first x-bin id */
    int32_t coord_bins;      /* 64  */
    int32_t pe_len;          /* 5000 */
    int32_t max_len;         /* 480: decode capacity (FORMAT_INFO['chartok_coords']['max_len']) */
    int32_t max_batch;       /* images per mnx_encode call the workspace is sized for */
    int32_t max_atoms;       /* kmax of mnx_edges (<= max_len / 3) */
    int32_t compute_dtype;   /* MNX_DTYPE_FP16X3 (fast AND reference-exact; the host side's default); MNX_DTYPE_BF16 = fastest */
    int32_t dec_slots;       /* sequences resident in the decoder during mnx_predict: multiple of 32, <= 4096; 0 = 2048 */
} mnx_config;

/* One named fp32 tensor of the checkpoint, in HOST memory. Names are the reference state-dict keys
 * ("transformer.layers.2.blocks.7.attn.qkv.weight", "decoder.chartok_coords.output_layer.bias", ...).
 * Index buffers (relative_position_index) and pe.pe are validated/recomputed, pass them or not. */
typedef struct {
    const char* name;
    const float* data;
    int32_t ndim;
    int64_t shape[4];
} mnx_weight_desc;

int mnx_abi_version(void);

/* Replaces `molnextr._get_model` + `loading` (MolNexTR/model.py:17-28,83-95): copies and packs the weights
 * into HBM (engine-owned), validates EVERY tensor of the contract by name and shape (the reference loads with
 * strict=False and ignores mismatches), and reserves all workspace for max_batch images — no allocation
 * happens after create. On failure *out is NULL and the message is available via mnx_last_error(NULL). */
int mnx_create(const mnx_config* cfg, const mnx_weight_desc* weights, int32_t n_weights, int32_t device,
               mnx_engine** out);
void mnx_destroy(mnx_engine* h);

/* NUL-terminated description of the last error on this handle (or of the last failed mnx_create if h==NULL). */
const char* mnx_last_error(const mnx_engine* h);
size_t mnx_workspace_bytes(const mnx_engine* h);

/* Replaces `Encoder.forward` -> `Vision_Transformer.forward` (MolNexTR/components.py:162-174,
 * MolNexTR/models/transformers.py:504-515). images: device fp32 [B,3,S,S] NCHW, normalised.
 * features_out: device fp32 [B, (S/32)^2, 8*embed_dim]. Asynchronous on `stream`. */
int mnx_encode(mnx_engine* h, const float* images, int32_t B, float* features_out, void* stream);

/* mnx_encode on the transform's gray bytes: gray device uint8 [B,S,S] (mnx_preprocess_batch with MNX_IMG_GRAY8; 4-byte
 * aligned). The patch embedding expands a byte g to the three channels (float(g) - 255 mean[c]) * (1 / (255 std[c])) — the
 * two fp32 operations the transform's fp32 output went through — so features_out equals mnx_encode's on the fp32 image of the
 * same bytes bit for bit. */
int mnx_encode_gray8(mnx_engine* h, const uint8_t* gray, int32_t B, float* features_out, void* stream);

/* Debug/test aid: copy the fp32 residual stream after execution item `item` of the next mnx_encode calls into
 * `dst` (device). Items: 0 = patch_embed, then every Swin block and every patch-merging in execution order.
 * item < 0 disables. */
int mnx_set_encoder_tap(mnx_engine* h, int32_t item, float* dst);

/* Test / measurement aid for the split modes (compute_dtype BF16X3 / FP16X3 / FP16X3M): choose per op class whether its
 * products are evaluated with the mode's own term count (bit set, the default: three, or two for the classes of
 * mnx_set_op_terms) or with the hi.hi term alone, i.e. as the plain 16-bit mode would. Bits: MNX_OP_* — 1 qkv Linear,
 * 2 window attention (QK^T and PV), 4 proj Linear, 8 fc1, 16 fc2, 32 patch-merging reduction.
 * Used by tests/test_gpu_pixels.py to measure which op classes the feature error comes from. No effect in other modes. */
int mnx_set_split_terms(mnx_engine* h, int32_t mask);

/* compute_dtype FP16X3 / FP16X3M only: the Linear op classes (MNX_OP_* bits, not MNX_OP_ATTN) of encoder stage `stage`
 * (0-based; -1 = every stage) that run on TWO terms (ah.wh + ah.wl) in the Swin blocks first_block .. last_block of the stage
 * (0-based, last_block may exceed the depth; the patch-merging reduction counts as the stage's last block). FP16X3 starts
 * with none, FP16X3M with MNX_FP16X3M_TWO_TERM_BY_STAGE from MNX_FP16X3M_FIRST_BLOCK_BY_STAGE on (an encoder of fewer than
 * four stages takes the table's last n_stages rows). two_term_mask = -1 reinstalls that starting table on `stage` (-1: every
 * stage; first_block / last_block are ignored). The weights are the same in both, so one engine can be measured under several tables
 * (tests/test_gpu_pixels.py; tools/study_split_terms.py is the CPU emulation). A 16-bit activation whose only consumer runs on
 * two terms is written as one plane. Takes effect at the next mnx_encode / mnx_predict call; not to be changed while one is
 * in flight. */
int mnx_set_op_terms(mnx_engine* h, int32_t stage, int32_t two_term_mask, int32_t first_block, int32_t last_block);

/* Synchronises `stream` and reports (then clears) whether any mnx_encode since the last call produced a non-finite
 * feature row — the only way the fp16 operand modes can fail on a checkpoint whose activations exceed 65504. */
int mnx_encoder_status(mnx_engine* h, int32_t* nonfinite, void* stream);

/* Replaces `TransformerDecoderAR.decode(beam_size=1)` (MolNexTR/components.py:253-334) including enc_transform
 * (:206-216), Embeddings with the batch-row positional-encoding quirk (MolNexTR/models/embedding.py:52-59),
 * TransformerDecoder stepwise forward (MolNexTR/models/decoder.py:431-486), output layer + log_softmax +
 * CharTokenizer.get_output_mask grammar (MolNexTR/tokenization.py:383-392) and GreedySearch
 * (MolNexTR/decoding/greedy_search.py:96-191).
 *   features   device fp32 [B,144,1024]                          B <= 32 per call
 *   chunk_id   device int32 [B] or NULL: rows with equal ids emulate ONE reference batch — row r gets the
 *              positional encoding of its rank among the still-undecoded rows of its chunk, as the reference
 *              does when it compacts finished rows out of the batch. NULL = all rows are one batch.
 *   max_len    <= cfg.max_len; rows stop at EOS or at max_len tokens (reference max_length)
 *   stop_on_eos 1 = reference behaviour; 0 = fixed-length decode (bench/test aid)
 *   tokens     device int32 [B,max_len]   ids without SOS, including EOS; entries >= lengths[b] are undefined
 *   lengths    device int32 [B]
 *   token_logp device fp32 [B,max_len] or NULL   log-prob of each emitted token (post-mask)
 *   hidden     device fp32 [B,max_len,256] or NULL   post-final-LayerNorm decoder outputs (input of mnx_edges)
 *   logits_trace device fp32 [max_len,B,vocab] or NULL (test aid: raw output_layer logits of every step)
 * Synchronous with respect to its outputs: returns after the last step has completed on `stream`. */
int mnx_decode_greedy(mnx_engine* h, const float* features, int32_t B, const int32_t* chunk_id, int32_t max_len,
                      int32_t stop_on_eos, int32_t* tokens, int32_t* lengths, float* token_logp, float* hidden,
                      float* logits_trace, void* stream);

/* Test aid: mnx_decode_greedy with TEACHER FORCING. Every row advances with forced_ids[b][t] (device int32 [B,max_len],
 * an id sequence that ends with EOS or fills max_len — e.g. the reference's own output) instead of its own argmax, so
 * the history, the finish steps and therefore the positional-encoding rows of the whole batch are the reference's at
 * every step. Outputs: argmax_ids [B,max_len] = what this engine would have chosen at each step GIVEN the reference
 * history; forced_logp [B,max_len] = masked log-prob it assigns to the forced id; lengths = steps taken; logits_trace as
 * mnx_decode_greedy. tests/test_gpu_pixels.py uses it to measure the log-prob error of the 16-bit operand modes along
 * the reference trajectory, free of knock-on effects, and to count argmax flips per token. */
int mnx_decode_forced(mnx_engine* h, const float* features, int32_t B, const int32_t* chunk_id, int32_t max_len,
                      const int32_t* forced_ids, int32_t* argmax_ids, int32_t* lengths, float* forced_logp,
                      float* logits_trace, void* stream);

/* LABEL-GUIDED greedy decoding: coordinate prediction for a KNOWN structure, `TransformerDecoderAR.decode(..., labels=...)`
 * (MolNexTR/components.py:253-334, the label handling at :284-332; decoding/greedy_search.py:76-127), which the reference
 * reaches from main.py --predict_coords with labels = smiles_to_sequence(smiles, mask_ratio=1) (dataset.py:459-464,
 * tokenization.py:429-462): every symbol a forced id, every atom's x and y '<mask>' (id 4). The guided sibling of
 * mnx_decode_greedy: the same arguments (stop_on_eos = 1) and
 *   labels     device int32 [B,L], L >= 2: column 0 '<sos>', a row ends with '<eos>' and is padded with '<pad>'; only the
 *              first min(L, max_len + 1) ids of a row are read (copied to an engine-owned table, one row per decode slot,
 *              allocated by the first guided call)
 * Semantics, per row b and step s:
 *   - the input of step s is labels[b][s] unless that is '<mask>', then the row's own pick of step s - 1; the grammar mask
 *     follows that mixed id (components.py:300-303); the EOS ban at step 0 and the max_len finish are mnx_decode_greedy's;
 *   - tokens[b][s] is the MERGED id: labels[b][s+1] unless that is '<mask>', then the own pick (components.py:331-332);
 *     token_logp[b][s] is the own argmax's masked log-prob, at forced positions too — not the forced id's
 *     (greedy_search.py:80,86; mnx_decode_forced differs in this); hidden is the model's own output of every step;
 *   - while s + 1 < L the row finishes iff labels[b][s+1] is '<eos>' — its own '<eos>' at a masked position does not finish
 *     it; finished rows leave the batch and the others' positional-encoding rows move up, labels travelling with their rows;
 *   - OURS: a row still alive at step L - 1 and beyond (its label holds no '<eos>', or max_len + 1 < L cut it) goes on
 *     free-running — own picks as input, finish on its own '<eos>' or at max_len — where the reference raises IndexError.
 * MNX_ERR_INVALID_ARG: labels NULL or L < 2; MNX_ERR_CAPACITY as mnx_decode_greedy. Synchronous with respect to its outputs. */
int mnx_decode_guided(mnx_engine* h, const float* features, int32_t B, const int32_t* chunk_id, int32_t max_len,
                      const int32_t* labels, int32_t L, int32_t* tokens, int32_t* lengths, float* token_logp, float* hidden,
                      float* logits_trace, void* stream);

/* Beam search over one reference batch — the `beam_size > 1` branch of TransformerDecoderAR.decode
 * (MolNexTR/components.py:253-334 with decoding/beam_search.py). The reference's own branch cannot run;
 * the strategy follows BeamSearch.advance/update_finished (beam_search.py:84-190: average log-prob over emitted
 * tokens + 2, flat top-k over beam x vocab, -1e10 for finished beams, stop when the top beam finished and n_best
 * hypotheses exist), the loop re-orders per step and tracks decoder outputs for the bond head (ours; documented in
 * DESIGN.md).
 *   features   device fp32 [B,144,1024], B <= 32 (one reference batch; PE row = row in the alive-images x beam batch)
 *   beam       1..8,  n_best 1..beam
 *   tokens     device int32 [B,n_best,max_len]  hypotheses by descending score; ids without SOS, EOS included
 *   lengths    device int32 [B,n_best]          (0 where fewer than n_best hypotheses finished — cannot happen when
 *                                                n_best <= beam, kept for robustness)
 *   scores     device fp32 [B,n_best]           average log-prob as defined above
 *   hidden     device fp32 [B,n_best,max_len,256] or NULL   decoder outputs along each hypothesis
 * Synchronous with respect to its outputs. */
int mnx_decode_beam(mnx_engine* h, const float* features, int32_t B, int32_t beam, int32_t n_best, int32_t max_len,
                    int32_t* tokens, int32_t* lengths, float* scores, float* hidden, void* stream);

/* Replaces the 'edges' branch of `Decoder.decode` (MolNexTR/components.py:470-491): GraphPredictor.forward
 * (:365-380), softmax over the 7 bond classes and get_edge_prediction (:383-400) incl. its float64 averaging.
 *   hidden   device fp32 [B,max_len,256] as written by mnx_decode_greedy
 *   atom_idx device int32 [B,kmax]: decoder position of each atom (CharTokenizer.sequence_to_smiles 'indices')
 *   n_atoms  device int32 [B]
 *   edges    device uint8 [B,kmax,kmax] bond class 0..6 (rows/cols >= n_atoms[b] are left as the caller filled them)
 *   scores   device fp64 [B,kmax,kmax] or NULL
 * B <= 32, kmax <= cfg.max_atoms. Device values out of range are read as clamped, never trusted: n_atoms[b] outside
 * 0..kmax as min(max(n_atoms[b], 0), kmax), atom_idx outside 0..max_len-1 as min(max(atom_idx, 0), max_len - 1).
 * Asynchronous on `stream`. */
int mnx_edges(mnx_engine* h, const float* hidden, const int32_t* atom_idx, const int32_t* n_atoms, int32_t B,
              int32_t kmax, int32_t max_len, uint8_t* edges, double* scores, void* stream);

/* The transform in front of the encoder (MolNexTR/dataset.py:158-185 with augment=False; data_aug.py:98-143,286-301;
 * applied per image at model.py:104): CropWhite(pad) [-> PadToSquare] -> Resize(img_size, bilinear) -> ToGray ->
 * Normalize -> CHW.
 *   rgb      device uint8 [height,width,3] (RGB, as cv2.cvtColor(BGR2RGB) leaves it)
 *   pad      white border added around the ink bounding box (the reference uses 50)
 *   pad_to_square  1 = insert PadToSquare after CropWhite, as `get_transforms` does for test files 'real/acs.csv' and
 *            'real/UOB.csv' (dataset.py:163-164): the shorter side is padded white, diff//2 before, the rest after
 *   crop_out device int32 [4] or NULL: {crop_top, crop_bottom, crop_left, crop_right} exactly as
 *            CropWhite.update_params computes them (data_aug.py:106-136) — pinned by tests/golden/crop_pad.json
 *   out      device fp32 [3,img_size,img_size] — one image of mnx_encode's input
 * Asynchronous on `stream`. Bit-identical to molnextr_amd/preprocess.py. CropWhite / PadToSquare are pinned on the
 * reference's own classes (golden crop boxes, shapes, content hashes); the OpenCV resize / gray arithmetic is restated
 * from its documented behaviour and held within 2 grey levels of exact bilinear interpolation (tests/test_gpu_prep_ref.py);
 * OpenCV's exact rounding inside that bound is unpinned (OpenCV is not installable here), see DESIGN.md. */
int mnx_preprocess(mnx_engine* h, const uint8_t* rgb, int32_t height, int32_t width, int32_t pad,
                   int32_t pad_to_square, int32_t* crop_out, float* out, void* stream);

/* The same transform for n pages in ONE call: three kernel launches whatever n (box init, boxes of all pages, resize of all
 * pages), no host synchronisation, no per-page host work, no host read of `pages`.
 *   arena      device bytes holding the pages as HWC uint8 RGB, page i at arena + pages[i].offset (any arena size: every
 *              address is 64-bit). The caller guarantees offset + 3 * height * width <= the arena's size.
 *   pages      DEVICE table of n entries; offset a multiple of 16, 1 <= height, width <= 16384 (the host never reads the
 *              table, so it cannot refuse an entry; one with height or width < 1 is transformed as a blank page)
 *   n          1 .. MNX_PREP_MAX_PAGES per call (the box scratch mnx_create reserved; MNX_ERR_CAPACITY beyond, the message
 *              names the bound); a longer list takes several calls
 *   max_height the tallest of the n pages (sizes the box kernel's grid; rows beyond it would not be scanned)
 *   crops_out  device int32 [n,4] or NULL: row i as mnx_preprocess's crop_out
 *   out        MNX_IMG_F32: device fp32 [n,3,S,S], word for word what n calls of mnx_preprocess write;
 *              MNX_IMG_GRAY8: device uint8 [n,S,S], the gray value in front of Normalize — the input of mnx_encode_gray8 /
 *              mnx_predict_gray8, a twelfth of the bytes (S = cfg.img_size)
 * MNX_ERR_INVALID_ARG: null pointer, n < 1, max_height outside 1..16384, pad outside 0..4096, unknown out_format, arena or
 * out misaligned (16 / 4 bytes). Asynchronous on `stream`. */
typedef struct {
    uint64_t offset;            /* bytes into `arena`, multiple of 16 */
    int32_t height, width;
} mnx_page;
enum { MNX_IMG_F32 = 0, MNX_IMG_GRAY8 = 1 };
#define MNX_PREP_MAX_PAGES 4096
int mnx_preprocess_batch(mnx_engine* h, const uint8_t* arena, const mnx_page* pages, int32_t n, int32_t max_height,
                         int32_t pad, int32_t pad_to_square, int32_t* crops_out, void* out, int32_t out_format,
                         void* stream);

/* Token classes for the on-device atom-position scan used by mnx_predict (the 'indices' that
 * CharTokenizer.sequence_to_smiles derives, MolNexTR/tokenization.py:464-515). flags[id]: bit0 = is_symbol(id),
 * bit1 = is_atom(id), bits 2-4 = length of the id's name in characters - 1 (read by the confidences only: an atom's
 * score spans as many ids as its symbol has characters, and '<unk>' is one id of five characters; 0 = one character)
 * for id < n (= number of vocabulary symbols); the ids of '[' ']' 'C' 'l' 'B' 'r'. */
int mnx_set_token_classes(mnx_engine* h, const uint8_t* flags, int32_t n, int32_t lbracket, int32_t rbracket,
                          int32_t id_C, int32_t id_l, int32_t id_B, int32_t id_r);

/* The atom-position scan on its own (test aid and building block of mnx_predict): tokens device int32 [n,T],
 * lengths device int32 [n] -> atom_idx device int32 [n,kmax], n_atoms device int32 [n]. */
int mnx_atom_scan(mnx_engine* h, const int32_t* tokens, const int32_t* lengths, int32_t n, int32_t T, int32_t kmax,
                  int32_t* atom_idx, int32_t* n_atoms, void* stream);

/* The whole hot path for a list of images, with continuous batching: replaces the body of the chunk loop of
 * `molnextr.predict_images` (MolNexTR/model.py:102-109: encoder + decoder.decode for every chunk) up to, but not
 * including, the host-side detokenisation to symbols / coordinates (mnx_graph_pack does that on the device, as a post-pass).
 *   images    device fp32 [n_img,3,S,S]
 *   ref_batch images are decoded as consecutive reference batches of this many rows, 1 <= ref_batch <=
 *             min(512, cfg.max_batch, cfg.dec_slots, cfg.pe_len) (MNX_ERR_CAPACITY otherwise; mnx_last_error names the
 *             bound): every batch is one positional-encoding numbering, exactly as if the reference had been called with
 *             this batch_size. A batch holds ceil(ref_batch / 32) tiles of 32 rows for as long as its longest row runs.
 * Up to cfg.dec_slots sequences (dec_slots / 32 row tiles; 2048 by default) are resident on the GPU at once;
 * every decode tick advances all of them by one token, finished batches are retired (atom positions + bond head run on device) and the freed rows are
 * refilled with the next batch while the encoder of the following batch runs on a second stream.
 *   stop_on_eos 1 = reference behaviour; 0 = every sequence runs to max_len (bench aid: deterministic decode work)
 *   tokens    device int32 [n_img,max_len]; lengths device int32 [n_img]
 *   n_atoms   device int32 [n_img]; atom_idx device int32 [n_img,kmax]; edges device uint8 [n_img,kmax,kmax]
 * Synchronous with respect to its outputs. */
int mnx_predict(mnx_engine* h, const float* images, int32_t n_img, int32_t ref_batch, int32_t max_len,
                int32_t stop_on_eos, int32_t* tokens, int32_t* lengths, int32_t* n_atoms, int32_t* atom_idx,
                uint8_t* edges, int32_t kmax, void* stream);

/* mnx_predict with the confidences of `Decoder.decode(compute_confidence=True)` (MolNexTR/components.py:456-469 atom
 * scores, :485-491 edge scores and overall score; decoding/greedy_search.py:109-110 token scores): the same inputs and
 * outputs (ref_batch up to 512 as there) with stop_on_eos = 1, and per image, all in the same continuous-batching pipeline (they are computed on the
 * device when a reference batch retires):
 *   token_logp    device fp32 [n_img,max_len] or NULL: masked log-prob of every emitted id, EOS included (0 beyond lengths)
 *   edge_scores   device fp64 [n_img,kmax,kmax]: probability of the chosen bond class, float64-averaged as in
 *                 get_edge_prediction (MolNexTR/components.py:383-400); rows / cols >= n_atoms are not written
 *   atom_scores   device fp64 [n_img,kmax]: geometric mean of exp(log-prob) over the ids that spell the atom's symbol
 *                 (as many ids back from its last one as the symbol has characters, Python slice semantics); 0 beyond n_atoms
 *   overall_score device fp64 [n_img]: exp(mean log-prob) * sqrt(product of edge_scores[0:n_atoms, 0:n_atoms])
 * Synchronous with respect to its outputs; reports MNX_ERR_RANGE as mnx_predict does. */
int mnx_predict_confidence(mnx_engine* h, const float* images, int32_t n_img, int32_t ref_batch, int32_t max_len,
                           int32_t* tokens, int32_t* lengths, int32_t* n_atoms, int32_t* atom_idx, uint8_t* edges,
                           int32_t kmax, float* token_logp, double* edge_scores, double* atom_scores, double* overall_score,
                           void* stream);

/* mnx_predict (the four confidence pointers all NULL) or mnx_predict_confidence (all four set; anything between is
 * MNX_ERR_INVALID_ARG) on gray bytes: gray device uint8 [n_img,S,S] as for mnx_encode_gray8, stop_on_eos = 1. The same
 * limits, MNX_ERR_RANGE reporting and continuous batching, and the same outputs bit for bit as on the fp32 images of the
 * same bytes. The format travels as an argument: a handle has no "current image format". Beam search stays on fp32 images
 * (mnx_predict_beam): out of scope here. */
int mnx_predict_gray8(mnx_engine* h, const uint8_t* gray, int32_t n_img, int32_t ref_batch, int32_t max_len,
                      int32_t* tokens, int32_t* lengths, int32_t* n_atoms, int32_t* atom_idx, uint8_t* edges, int32_t kmax,
                      float* token_logp, double* edge_scores, double* atom_scores, double* overall_score, void* stream);

/* The continuous-batching pipeline with LABELS: main.py --predict_coords of the reference (dataset.py:459-464 makes the
 * labels, components.py:284-332 and greedy_search.py:76-127 decode along them, components.py:452-491 derives atoms, bonds and
 * confidences from the merged ids, the own-pick scores and the own decoder outputs). Inputs and outputs of mnx_predict_gray8,
 * every row decoded as mnx_decode_guided defines (its free-running extension beyond L included):
 *   images     img_format MNX_IMG_F32: device fp32 [n_img,3,S,S]; MNX_IMG_GRAY8: device uint8 [n_img,S,S], 4-byte aligned.
 *              The format travels as an argument; both give the same outputs bit for bit on the same bytes.
 *   ref_batch  up to 512 under mnx_predict's capacity rules
 *   labels     device int32 [n_img,L], L >= 2, row i belongs to image i; min(L, max_len + 1) ids of a row are copied to the
 *              engine's per-slot label table on the decode stream when its reference batch is admitted (the table,
 *              dec_slots x (cfg.max_len + 2) ids, is allocated by the first guided call and kept until mnx_destroy)
 *   the four confidence pointers: all NULL or all set, as for mnx_predict_gray8
 * Guided ticks replay graphs of their own; a guided job never invalidates the graphs of unguided ones.
 * MNX_ERR_INVALID_ARG: labels NULL, L < 2, unknown img_format, misaligned gray, confidence pointers partly set;
 * MNX_ERR_CAPACITY and MNX_ERR_RANGE as mnx_predict. Synchronous with respect to its outputs. */
int mnx_predict_guided(mnx_engine* h, const void* images, int32_t img_format, int32_t n_img, int32_t ref_batch,
                       int32_t max_len, const int32_t* labels, int32_t L, int32_t* tokens, int32_t* lengths, int32_t* n_atoms,
                       int32_t* atom_idx, uint8_t* edges, int32_t kmax, float* token_logp, double* edge_scores,
                       double* atom_scores, double* overall_score, void* stream);

/* The confidence computation on its own (test aid and building block of mnx_predict_confidence; replaces the
 * compute_confidence lines of MolNexTR/components.py:456-469,485-491): tokens device int32 [n,T] (T <= 512), lengths
 * device int32 [n], token_logp device fp32 [n,T], atom_idx device int32 [n,kmax] and n_atoms device int32 [n] (as the
 * atom scan writes them), edge_scores device fp64 [n,kmax,kmax] -> atom_scores device fp64 [n,kmax], overall_score device
 * fp64 [n], defined as for mnx_predict_confidence. Deterministic (fixed-order reductions). Asynchronous on `stream`. */
int mnx_confidence(mnx_engine* h, const int32_t* tokens, const int32_t* lengths, const float* token_logp, int32_t n,
                   int32_t T, const int32_t* atom_idx, const int32_t* n_atoms, const double* edge_scores, int32_t kmax,
                   double* atom_scores, double* overall_score, void* stream);

/* The names of the vocabulary's symbol ids, for mnx_graph_pack: the name of id i is bytes[offsets[i] .. offsets[i+1]), UTF-8,
 * at most 8 bytes, for i < n; n must be cfg.sym_offset (at most 256): one name for every symbol id, so that no id is spelled
 * as nothing. The reference vocabulary holds the five specials '<pad>' .. '<mask>' and one two-byte character; every other
 * name is one byte. Copied to the device (host pointers, read before the call returns): the sibling of mnx_set_token_classes.
 * MNX_ERR_INVALID_ARG (with mnx_last_error): null pointer, n outside 1..256, offsets[0] != 0, a name of more than 8 bytes or
 * a decreasing offset, n != cfg.sym_offset. */
int mnx_set_vocab_text(mnx_engine* h, const char* bytes, const uint32_t* offsets, int32_t n);

/* Molecules as packed tables: the dense outputs of any mnx_predict* call (or of mnx_atom_scan / mnx_edges / mnx_confidence)
 * turned on the device into what CharTokenizer.sequence_to_smiles (MolNexTR/tokenization.py:464-515) and the pair loop of
 * predict_images (MolNexTR/model.py:135-143) derive from them on the host — per image the raw token SMILES, one record per
 * atom and one per bond — so that a caller copies a few hundred bytes per image and needs no tokenizer of its own.
 * A post-pass: it reads the outputs of mnx_predict*, changes none of them and touches no decode state.
 *
 * The three record types (natural C layout, no packing pragma; records are written whole, padding bytes as zeros):
 *   struct mnx_mol, 40 bytes   atom0, bond0, text0: where the image's atoms / bonds / SMILES start in `atoms`, `bonds`, `text`
 *                              (the tables of image b lie behind those of image b - 1); n_atoms, n_bonds, smiles_len: how many;
 *                              flags bit 0: the token walk found more atoms than kmax and the tables hold the first kmax;
 *                              overall_score (0 without scores)
 *   struct mnx_atom, 24 bytes  the symbol is the sym_len bytes at text + text0 + sym0 (an atom's symbol is a substring of its
 *                              molecule's SMILES: no second copy); index = its decoder position (atom_idx, the tokenizer's
 *                              'indices'); x_bin, y_bin: the coordinate is bin / (cfg.coord_bins - 1), computed by the consumer
 *                              in double — the reference's own Python division; score = atom_scores (0 without scores)
 *   struct mnx_bond, 16 bytes  i < j; type = edges[i][j], rev = edges[j][i]; one record for every edges[i][j] != 0 with
 *                              i < j < n_atoms, i ascending, then j ascending; score = edge_scores[i][j] (0 without scores)
 * Inputs, device pointers exactly as mnx_predict* writes them: tokens int32 [n,T], lengths int32 [n], atom_idx int32 [n,kmax],
 * n_atoms int32 [n], edges uint8 [n,kmax,kmax]; atom_scores fp64 [n,kmax], edge_scores fp64 [n,kmax,kmax], overall_score fp64
 * [n]: all three or none. 1 <= n <= 65536, 1 <= T <= 512, 1 <= kmax <= cfg.max_atoms. The atoms come from the atom scan's own
 * token walk over the ids (their count is min(walk, kmax)); bonds are read among the first min(that, n_atoms[b]) atoms.
 * Outputs, device pointers the caller allocated: mols [n]; atoms [atom_cap], bonds [bond_cap] (8-byte aligned), text
 * [text_cap] bytes (no terminators); totals uint32 [4] = {atoms, bonds, text bytes needed, 1 if any capacity was too small}.
 * When a capacity is too small nothing is written beyond it, and mols and totals are complete all the same: read the needed
 * sizes and call again. Deterministic word for word (every position comes from a prefix scan; no atomics). Three launches,
 * asynchronous on `stream`, no allocation, no host synchronisation.
 * MNX_ERR_INVALID_ARG (with mnx_last_error, "mnx_graph_pack: ..."): a null pointer (a table with capacity 0 may be null), a
 * size outside the limits, the scores partly set, misaligned records, or no vocabulary text / token classes set. */
typedef struct mnx_mol {
    uint32_t atom0, n_atoms, bond0, n_bonds, text0, smiles_len;
    uint32_t flags;             /* bit 0: more atoms than kmax, tables truncated to kmax; MNX_MOL_EXPAND* of mnx_expand_pack; bits 4-6 of mnx_normalize_pack; bits 7-9 of mnx_kekulize_pack; bits 10, 11, 16, 17 of mnx_formula_pack; bits 18-20 of mnx_main_pack */
    uint32_t reserved;          /* 0 */
    double overall_score;
} mnx_mol;
typedef struct mnx_atom {
    uint32_t sym0;              /* bytes from the molecule's text0 */
    uint16_t sym_len, index, x_bin, y_bin;
    double score;
} mnx_atom;
typedef struct mnx_bond {
    uint16_t i, j;
    uint8_t type, rev;
    double score;
} mnx_bond;
#define MNX_MOL_TRUNCATED 1u
int mnx_graph_pack(mnx_engine* h, const int32_t* tokens, const int32_t* lengths, int32_t n, int32_t T,
                   const int32_t* atom_idx, const int32_t* n_atoms, const uint8_t* edges, int32_t kmax,
                   const double* atom_scores, const double* edge_scores, const double* overall_score, mnx_mol* mols,
                   mnx_atom* atoms, uint32_t atom_cap, mnx_bond* bonds, uint32_t bond_cap, char* text, uint32_t text_cap,
                   uint32_t* totals, void* stream);

/* The R-group and abbreviation names that _convert_graph_to_smiles tests an atom's symbol against before it reads it as a
 * chemical element (MolNexTR/chemical.py:886-895, the tables of abbrs.py), for mnx_molfile_pack: name i is
 * bytes[offsets[i] .. offsets[i+1]), 1..16 bytes, kinds[i] = 1 for an R-group and 2 for an abbreviation; n <= 512 names,
 * strictly ascending bytewise (unsigned bytes; a prefix sorts in front of the longer name), so that the device finds a name
 * by binary search. A name that is in both of the reference's tables ('Z') is listed once, as an R-group: that table is
 * tested first. Copied to the device (host pointers, read before the call returns): a sibling of mnx_set_vocab_text.
 * MNX_ERR_INVALID_ARG (with mnx_last_error): null pointer, n outside 0..512, offsets[0] != 0, a name of 0 or more than 16
 * bytes, names not strictly ascending, a kind other than 1 or 2. A call drops the fragments of an earlier mnx_set_fragments
 * (they are parallel to the names): set them again. */
int mnx_set_symbol_tables(mnx_engine* h, const char* bytes, const uint32_t* offsets, const uint8_t* kinds, int32_t n);

/* Molecules as CTfile V2000 molfiles, written on the device from the tables of mnx_graph_pack: the molecule that
 * _convert_graph_to_smiles puts together with RDKit (MolNexTR/chemical.py:880-926: atoms by symbol class, bonds with their
 * wedge classes), at the coordinates it hands to _verify_chirality (:935-939: x * ratio * 10, y * 10, y pointing up) and with
 * the begin atom of a wedge moved to the chiral centre as :262-273 do. No SMILES (that needs RDKit's canonicaliser) and no
 * abbreviation expansion (that is mnx_expand_pack, in front of this call). The format follows the CTfile specification; it is
 * this library's own and not RDKit's writer byte for byte. A post-pass on a post-pass: it reads mols / atoms / bonds / text as mnx_graph_pack wrote them (device pointers,
 * with the numbers of records / bytes those tables hold), changes none of them and touches no decode state.
 *
 * One atom, from the sym_len bytes of its symbol, in the reference's order of tests: one pair of enclosing '[' ']' is
 * stripped; the inner text in the R-group table, or else in the abbreviation table, makes a pseudo-atom; else the WHOLE
 * symbol is read as a SMILES atom — unbracketed B C N O P S F Cl Br I, b c n o p s, '*'; bracketed
 * isotope? (element | b c n o p s se as | '*') ('@' | '@@')? ('H' digit?)? charge? (':' digits)?, element one of the 118
 * symbols (longest match), charge a run of '+' or of '-' or one sign and a number, |charge| <= 15, isotope <= 999 —; what does
 * not parse is a pseudo-atom too. The chirality mark is read and dropped (the reference clears the tag: stereo travels as
 * wedges and coordinates).
 *
 * One molfile (every line ends with '\n'; no timestamp, so the bytes are deterministic):
 *   header   an empty line, "  MolNexTR          2D", an empty line
 *   counts   "%3d%3d  0  0  0  0  0  0  0  0999 V2000"
 *   atom     "%10.4f%10.4f%10.4f %-3s 0  0  0  0  0%3d  0  0  0  0  0  0" (69 bytes), z = 0.0000. x and y in exact integer
 *            arithmetic, in units of 1e-4: den = cfg.coord_bins - 1, bins clamped to 0..den,
 *            ux = (2 * x_bin * Sx + den) / (2 * den), uy = (2 * (den - y_bin) * Sy + den) / (2 * den) (64-bit integer
 *            division), printed as u / 10000 '.' u % 10000 (four digits). Symbol: the element, capitalised for aromatic
 *            atoms; "R#" for an R-group named 'R' + a number 1..999; "R" for every other pseudo-atom and for '*'. A '*' that parses ('*', '[*]',
 *            '[*+]') is an atom of the grammar whose symbol happens to be "R": it has no alias, keeps its charge and isotope
 *            in M  CHG / M  ISO, and does NOT count as a pseudo-atom for flag bit 2. The %3d is
 *            the valence field: for a parsed BRACKET atom without an aromatic bond H count + the sum of its bond orders
 *            (classes 1, 5, 6 count 1, class 2 two, class 3 three), written as 15 when that is 0 and as 0 when it exceeds 14;
 *            0 for every other atom. Known limit: a bracket atom on an aromatic bond ('[nH]') loses its hydrogen mark.
 *   bond     "%3d%3d%3d%3d" (12 bytes), atoms 1-based: classes 1..4 are type 1..4 with stereo 0, classes 5 / 6 type 1 with
 *            stereo 1 / 6 (any other class: type 8, stereo 0). When atom j's symbol is exactly one of [C@] [C@@] [C@H] [C@@H]
 *            and `rev` is 5 or 6 the line reads j i with rev's type and stereo, otherwise i j with type's.
 *   properties, in this order: "A  %3d" + a line with the inner symbol (at most 70 bytes, cut at a UTF-8 character boundary;
 *            control bytes as '?') for every pseudo-atom from the tables or without a parse whose inner symbol is not empty;
 *            "M  CHG", "M  ISO" (the isotopes of [13C] and the like), "M  RGP" (the numbers of the "R#" atoms), each as
 *            "M  XXX%3d" + up to eight " %3d %3d" pairs per line, atoms ascending; "M  END".
 *
 *   struct mnx_molfile, 16 bytes  text0, len: the molecule's molfile is out[text0 .. text0 + len); flags bit 0: more than 999
 *            atoms or bonds; bit 1: a record points beyond a table — atom0 + n_atoms, bond0 + n_bonds or text0 + smiles_len
 *            beyond the sizes passed (a mnx_graph_pack output that was cut at a capacity, say), an atom's symbol beyond
 *            n_text_bytes, a bond whose i or j is not an atom of the molecule —; either bit: no molfile, len = 0. Bit 2: the
 *            molecule holds a pseudo-atom; bit 3: a copy of MNX_MOL_TRUNCATED.
 * Inputs: mols [n], 1 <= n <= 65536; atoms [n_atom_records], bonds [n_bond_records] (8-byte aligned), text [n_text_bytes];
 * scale device int32 [n,2] = {Sx, Sy} of every molecule in units of 1e-4, each 1..10 000 000, or NULL for Sx = Sy = 100000
 * (the reference's factor 10 on a square page; Sx = round(100000 * width / height) gives its `ratio`). scale is device
 * memory, which a host call cannot read without a synchronisation: a value outside the range is clamped by the kernel.
 * mnx_set_symbol_tables must have been called.
 * Outputs, device pointers the caller allocated: files [n]; out [out_cap] bytes (no terminators); totals uint32 [2] = {bytes
 * needed, 1 if out_cap was too small}. Nothing is written beyond out_cap, and files and totals are complete all the same:
 * read the needed size and call again. Deterministic byte for byte (every position comes from a prefix scan; no atomics).
 * Three launches, asynchronous on `stream`, no allocation, no host synchronisation.
 * MNX_ERR_INVALID_ARG (with mnx_last_error, "mnx_molfile_pack: ..."): a null pointer (a table of size 0 may be null), n
 * outside 1..65536, misaligned records, or no symbol tables set; nothing is launched then. */
typedef struct mnx_molfile {
    uint32_t text0, len;
    uint32_t flags;             /* MNX_MOLFILE_* */
    uint32_t reserved;          /* 0 */
} mnx_molfile;
#define MNX_MOLFILE_TOO_LARGE 1u
#define MNX_MOLFILE_BEYOND_TABLES 2u
#define MNX_MOLFILE_PSEUDO_ATOM 4u
#define MNX_MOLFILE_TRUNCATED 8u
int mnx_molfile_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                     const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes,
                     const int32_t* scale, mnx_molfile* files, char* out, uint32_t out_cap, uint32_t* totals, void* stream);

/* Molecules as SMILES of the predicted GRAPH, written on the device from the tables of mnx_graph_pack: the atoms of the token
 * string joined by the bonds of the bond head — the raw token SMILES in `text` names the atoms but its bonds can disagree
 * with `bonds`. The string is VALID after the OpenSMILES grammar and NOT canonical (the walk below is fixed by the atom
 * indices; any toolkit can canonicalise it); it carries no stereo ('@', '/', '\' are never written by this call: wedges are
 * dropped; mnx_smiles_pack_stereo and mnx_smiles_pack_marks below write them) and
 * expands no abbreviation (a pseudo-atom is '*'). The third post-pass after mnx_graph_pack and mnx_molfile_pack, with the
 * arguments, limits and error handling of the latter; it changes no input and touches no decode state.
 *
 * One atom is read exactly as mnx_molfile_pack reads it (brackets stripped, R-group table, abbreviation table, then the whole
 * symbol through the bracket-atom grammar stated there) and written as
 *   a parsed unbracketed atom (B C N O P S F Cl Br I, b c n o p s, '*'): its bytes as they are;
 *   a parsed bracket atom: '[' isotope-if-nonzero, the element as spelled (lower case is kept: that is what makes an atom
 *     aromatic), 'H' for one hydrogen or 'H' digit for more, the charge ('+' / '-' for +-1, else the sign and the decimal
 *     magnitude), ']'; the chirality mark and the ':class' are dropped: [C@@H] -> [CH], [N++] -> [N+2], [C:12] -> [C],
 *     [nH] stays [nH];
 *   a pseudo-atom (a table name, or no parse): "[k*]" for an R-group named 'R' + a number k in 1..999 (the reference sets
 *     that isotope on its '*' atom), '*' for every other; flag bit 2 is set as in the molfile; nothing is expanded.
 * One bond is an unordered pair whose class is `type` (`rev` is ignored): 1, 5, 6 single; 2 '='; 3 '#'; 4 aromatic; any other
 * '~'. A single bond is written as nothing, but as '-' between two aromatic (lower-case) atoms; an aromatic bond as nothing
 * between two aromatic atoms and as ':' otherwise.
 * The walk: components in the order of their lowest atom index, joined by '.'; depth-first from that atom, an atom's
 * neighbours in ascending atom index; an unvisited neighbour becomes a child, every other bond that is not the bond to the
 * parent is a ring bond. Behind an atom's own text stand its ring bonds, then its children in ascending index, every child but
 * the last inside '(' ')', the bond symbol of a child directly in front of its atom (inside the parenthesis).
 * Ring closure numbers, atoms taken in written order: at an atom first every ring bond whose other end was written earlier, in
 * ascending written position of that end, as the number it was allotted (no bond symbol); then every ring bond whose other
 * end comes later, in ascending written position of that end, as the bond symbol and the lowest free number >= 1. The numbers
 * an atom closes are free from the next atom on (no number appears twice at one atom). 1..9 are a digit, 10..99 '%nn'; a
 * molecule that would hold more than 99 numbers at once gets no SMILES.
 *
 *   struct mnx_smiles, 16 bytes  text0, len: the molecule's SMILES is out[text0 .. text0 + len); flags (MNX_SMILES_*): bit 0 more
 *            than 999 atoms or bonds; bit 1 a record beyond the tables (the cases mnx_molfile_pack lists) or a bond with
 *            i == j; bit 2 the molecule holds a pseudo-atom; bit 3 a copy of MNX_MOL_TRUNCATED; bit 4 the same atom pair in two
 *            bond records; bit 5 more than 99 ring numbers in use; bit 6 a bond of class 5 or 6 was written as a plain single
 *            bond; bit 7 a bond of an unknown class was written as '~'. On bits 0, 1, 4 or 5 the molecule gets no SMILES:
 *            len = 0, and bits 6 and 7 stay clear (nothing was written). n_rings: the ring bonds = bonds - atoms + components
 *            (0 on bits 0 and 1, whose records are not read). An empty molecule has len = 0 and flags = 0.
 * Inputs: as mnx_molfile_pack (mols [n], 1 <= n <= 65536; atoms, bonds 8-byte aligned; text; the sizes of the three tables);
 * the molecules' atom ranges must not overlap. mnx_set_symbol_tables must have been called.
 * Outputs, device pointers the caller allocated: recs [n]; order uint16 [n_atom_records] or NULL: order[atom0 + k] = the 0-based
 * position of the molecule's atom k among the atoms of its string (to carry coordinates and scores over to SMILES atom
 * order), 0xFFFF for every atom of a molecule that gets no SMILES (entries of atoms outside the table, and of no molecule,
 * are not written); out [out_cap] bytes (no terminators, no separators); totals uint32 [2] = {bytes needed, 1 if out_cap was
 * too small}. Nothing is written beyond out_cap, and recs, order and totals are complete all the same: read the needed size
 * and call again; a sizing call may pass out = NULL with out_cap = 0. Deterministic byte for byte (every output position
 * comes from a prefix scan; no atomic decides a position or an order). Three launches, asynchronous on `stream`, no
 * allocation, no host synchronisation.
 * MNX_ERR_INVALID_ARG (with mnx_last_error, "mnx_smiles_pack: ..."): a null pointer (a table of size 0 and `order` may be
 * null), n outside 1..65536, misaligned records, or no symbol tables set; nothing is launched then. */
typedef struct mnx_smiles {
    uint32_t text0, len;
    uint32_t flags;             /* MNX_SMILES_* */
    uint32_t n_rings;
} mnx_smiles;
#define MNX_SMILES_TOO_LARGE 1u
#define MNX_SMILES_BEYOND_TABLES 2u
#define MNX_SMILES_PSEUDO_ATOM 4u
#define MNX_SMILES_TRUNCATED 8u
#define MNX_SMILES_DUPLICATE_BOND 16u
#define MNX_SMILES_RING_NUMBERS 32u
#define MNX_SMILES_WEDGES_DROPPED 64u
#define MNX_SMILES_UNKNOWN_BOND 128u
int mnx_smiles_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                    const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_smiles* recs,
                    uint16_t* order, char* out, uint32_t out_cap, uint32_t* totals, void* stream);

/* mnx_smiles_pack with tetrahedral stereo marks: the same arguments, limits, error handling, sizing protocol and three
 * launches, and the same string with ONE change — a candidate centre that resolves is written as [C@], [C@@], [C@H] or [C@@H]
 * instead of [C] / [CH]. Removing every '@' from the string gives the string of mnx_smiles_pack byte for byte; `order` and
 * n_rings are those of the plain call, len grows by 1 or 2 per mark. mnx_smiles_pack itself is unchanged. No '/' '\' at double
 * bonds here: mnx_smiles_pack_marks below writes them. The rule is this library's own, after the OpenSMILES definition of '@' / '@@' and the reference's "a wedge begins at
 * the marked carbon" (_verify_chirality, MolNexTR/chemical.py:212-287: bond directions cleared, put back only at atoms whose
 * token is one of the four symbols, as edges[c][n] seen from that atom; the 2D coordinates decide; every other tag cleared). It
 * is NOT RDKit's AssignChiralTypesFromBondDirs: in degenerate drawings (neighbours on one line, a wedge between two
 * neighbours that lie on a line through the centre) the two can differ. No symmetry check is made HERE: a carbon with four
 * identical substituents is marked like one with four different ones; mnx_smiles_pack_symmetric below drops the marks of
 * centres with two substituents of one symmetry class.
 *
 * Candidate centre: an atom c for which all of these hold —
 *   its symbol is exactly one of [C@] [C@@] [C@H] [C@@H] (the test of mnx_molfile_pack's bond lines) and is read as an atom
 *     (it is no name of the symbol tables); H = 0 for [C@] [C@@], 1 for [C@H] [C@@H];
 *   the number of its bond records + H = 4;
 *   every one of its bonds has written class single (`type` 1, 5 or 6);
 *   at least one of its bonds is a wedge SEEN FROM c. The class of a bond seen from c is `type` when c == i and `rev` when
 *     c == j (edges[c][n]). Seen class 5 puts neighbour n at z = +1 (towards the viewer), seen class 6 at z = -1, every other
 *     seen class at z = 0.
 * Geometry: the vector of neighbour n is v(n) = (x_bin[n] - x_bin[c], y_bin[c] - y_bin[n], z) — the image's y axis points
 *   down, the vector has y up. Exact 64-bit integer arithmetic; no scale (the sign depends neither on a positive scale of x
 *   nor on the magnitude of z). The '@' or '@@' of the symbol itself is ignored: the mark comes from the drawing alone.
 * Neighbour order of the string at c: the parent if c has one; then the implicit H if H = 1; then c's ring items in the order
 *   they are written at c (closures, then openings, as stated above); then its children in written order.
 * Four explicit neighbours n0..n3 in that order: d = det[v1 - v0, v2 - v0, v3 - v0] (the rows of a 3x3 determinant).
 * Three explicit neighbours n0..n2 in that order: d = det[v0, v1, v2], negated when the H stands at an odd position of the
 *   four — position 1, behind a parent; the H stands at position 0 only when c starts a component.
 * Mark: d < 0 writes '@', d > 0 writes '@@' (directly behind the 'C'), d == 0 writes no mark.
 * Examples (atoms with (x_bin, y_bin), bonds (i, j, type, rev)):
 *   F(20,30) [C@@](20,20) Cl(20,10) Br(11,25) I(29,25), (0,1,6,5) (1,2,1,1) (1,3,1,1) (1,4,1,1)   ->  F[C@](Cl)(Br)I
 *   N(10,20) [C@H](20,20) C(25,11) C(25,29) O(20,38) O(35,29), (0,1,1,1) (1,2,5,6) (1,3,1,1) (3,4,2,2) (3,5,1,1)
 *                                                            ->  N[C@@H](C)C(=O)O, and with (1,2,6,5)  ->  N[C@H](C)C(=O)O
 *   [C@H](20,20) C(30,26) C(30,14) F(10,20), (0,1,1,1) (0,2,1,1) (1,2,1,1) (0,3,5,6)               ->  [C@H]1(CC1)F
 *
 * Flags: bits 0-5 and 7 as in mnx_smiles_pack. Bit 6 (MNX_SMILES_WEDGES_DROPPED) is set only when some bond with `type` 5 or 6
 * has NO end that received a mark; bit 8 (MNX_SMILES_STEREO) when at least one mark was written; bit 9
 * (MNX_SMILES_STEREO_UNRESOLVED) when an atom with one of the four symbols and a wedge seen from it got no mark (the neighbour
 * count, a bond that is not single, or d == 0). All three stay clear on a molecule that gets no SMILES.
 * MNX_ERR_INVALID_ARG as mnx_smiles_pack, the text beginning "mnx_smiles_pack_stereo: ". */
#define MNX_SMILES_STEREO 256u
#define MNX_SMILES_STEREO_UNRESOLVED 512u
int mnx_smiles_pack_stereo(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                           const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes,
                           mnx_smiles* recs, uint16_t* order, char* out, uint32_t out_cap, uint32_t* totals, void* stream);

/* mnx_smiles_pack with the marks the caller selects: the arguments of mnx_smiles_pack and `marks`, a set of MNX_SMILES_MARK_*,
 * in front of `stream`; the same limits, sizing protocol (`totals`), `order`, refusal cases and three launches.
 *   marks == 0                              the bytes, order, records and flags of mnx_smiles_pack
 *   marks == MNX_SMILES_MARK_TETRAHEDRAL    those of mnx_smiles_pack_stereo
 *   marks == MNX_SMILES_MARK_DOUBLE_BOND    '/' and '\' at double bonds, by the rule below
 *   both                                    both kinds of marks, each by its own rule: neither looks at the other
 * Any other bit is MNX_ERR_INVALID_ARG and nothing is launched. The two older calls are unchanged.
 * Invariants: removing every '/' and '\' from the string of marks == 2 (and putting back the '-' where one of them replaced it
 * between two aromatic atoms) gives the bytes of mnx_smiles_pack, and from marks == 3 those of mnx_smiles_pack_stereo; removing
 * every '@' from marks == 3 gives marks == 2; `order` and n_rings never change, len grows by 1 per symbol written in front of
 * an atom that had none and stays where a '-' is replaced.
 *
 * The rule of '/' and '\' is this library's own, after the OpenSMILES reading of the two symbols and the reference's way of
 * taking double-bond E/Z from the 2D coordinates (_verify_chirality, MolNexTR/chemical.py:212-287: AssignStereochemistryFrom3D
 * on the flat conformer). It is NOT RDKit's. No toolkit has parsed the output. No symmetry check is made HERE: FC(F)=C(F)F is marked
 * like any other double bond; mnx_smiles_pack_symmetric below drops the marks of such bonds. Known limit: a double bond on a
 * cycle of the molecule's bond graph is never marked, a macrocycle's included.
 *
 * Candidate: a bond record with `type` 2 for which all of these hold —
 *   it lies on no cycle of the molecule's bond graph;
 *   both its ends are read as atoms, not pseudo-atoms;
 *   each end has 1 or 2 further bond records;
 *   all of those have written class single (`type` 1, 5 or 6).
 *   A candidate is therefore always a tree bond of the walk: a is its end written earlier, b (a's child) the other.
 * Geometry, exact integers on the bins, y up (the image's y points down): the axis A = (x_bin[b] - x_bin[a], y_bin[a] - y_bin[b]);
 *   a substituent s of the end u (u = a or b; every atom bonded to u but the other end) has v = (x_bin[s] - x_bin[u],
 *   y_bin[u] - y_bin[s]) and side(s) = sign(A.x * v.y - A.y * v.x), with the same A at both ends: +1 is left of a -> b.
 * Resolved: no substituent has side 0, and where an end has two substituents their sides are opposite. Substituents on ring
 *   bonds count here. A candidate that does not resolve writes no marks (bit 11).
 * Where the symbols go: only on tree bonds of the walk — the bond from a's parent to a, and the bonds from a and from b to
 *   their children other than a -> b. The symbol stands in front of the child atom, where the bond's symbol stands (inside the
 *   parenthesis), and replaces nothing, or the '-' between two aromatic atoms. A ring bond (a ring-closure digit) never
 *   carries one. Every end of a candidate has at least one substituent on a tree bond, so every resolved candidate is marked
 *   at both ends.
 * Which symbol: with up(s) = (side(s) > 0) XOR flip, the candidate's flip being the same for all its substituents,
 *   the bond u -> s to a child s of u = a or b is written '/' when up(s), else '\';
 *   the bond p -> a from a's parent p is written '\' when up(p), else '/'.
 * The flip: resolved candidates are taken in ascending written position of a. A candidate's directed bonds are listed as (1)
 *   the bond from a's parent, (2) the bonds to a's other children in written order, (3) the bonds to b's children in written
 *   order. If (1) exists and an earlier candidate (one that a's parent is an end of) already gave it a symbol, flip is the value
 *   that reproduces that symbol; otherwise flip is the value that makes the first bond of the list '/'. Only (1) can have a
 *   symbol already; these constraints run along tree bonds, so they form a forest and cannot conflict.
 * Examples (atoms with (x_bin, y_bin), bonds (i, j, type, rev)):
 *   F(0,20) C(10,10) C(20,10) F(30,0), (0,1,1,1) (1,2,2,2) (2,3,1,1)                    ->  F/C=C/F
 *   the same with the last F at (30,20)                                                 ->  F/C=C\F
 *   C(0,20) C(10,10) C(20,20) C(30,10) C(40,20) C(50,10), (0,1,1,1) (1,2,2,2) (2,3,1,1) (3,4,2,2) (4,5,1,1)
 *                                                                                       ->  C/C=C/C=C/C
 *   C(0,10) C(10,10) C(20,0) C(30,0) C(40,10) C(30,20) C(20,20) F(0,0), (0,1,2,2) (1,2,1,1) (2,3,1,1) (3,4,1,1) (4,5,1,1)
 *   (5,6,1,1) (1,6,1,1) (0,7,1,1)                                                       ->  C(=C1/CCCCC1)/F
 *
 * Flags: bits 0-9 as the call with the same MNX_SMILES_MARK_TETRAHEDRAL bit gives them. Bit 10 (MNX_SMILES_EZ): at least one
 * '/' or '\' was written. Bit 11 (MNX_SMILES_EZ_UNRESOLVED): a candidate got no marks. Bit 12 (MNX_SMILES_EZ_IMPLIED): a bond
 * record with `type` 2 that is no resolved candidate has, at each of its two ends, a bond that carries a symbol — a reader
 * takes a configuration from there that the drawing did not give; the caller can fall back to the string without double-bond
 * marks for that molecule. All three stay clear on a molecule that gets no SMILES and without MNX_SMILES_MARK_DOUBLE_BOND.
 * MNX_ERR_INVALID_ARG as mnx_smiles_pack, the text beginning "mnx_smiles_pack_marks: ". */
#define MNX_SMILES_MARK_TETRAHEDRAL 1u
#define MNX_SMILES_MARK_DOUBLE_BOND 2u
#define MNX_SMILES_EZ 1024u
#define MNX_SMILES_EZ_UNRESOLVED 2048u
#define MNX_SMILES_EZ_IMPLIED 4096u
int mnx_smiles_pack_marks(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                          const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes,
                          mnx_smiles* recs, uint16_t* order, char* out, uint32_t out_cap, uint32_t* totals, uint32_t marks,
                          void* stream);

/* mnx_smiles_pack_marks on CANONICAL ATOM RANKS: a string that does not depend on how the atoms of a drawing are numbered or
 * its bond records ordered. The arguments of mnx_smiles_pack_marks and two more outputs, `rank` and `sym_class`; the same
 * limits, sizing protocol (`totals`), refusal cases and `marks` (0..3; any other bit is MNX_ERR_INVALID_ARG). The older calls
 * are unchanged. The ranking is this library's own (a partition refinement after Morgan / Weininger) and it is NOT RDKit's
 * canonical SMILES, nor any other toolkit's: no toolkit has parsed the output, two libraries' canonical strings never compare,
 * and scores against canonicalised gold strings still need a toolkit. It serves to deduplicate, count agreeing predictions
 * and key a cache on a host without one.
 *
 * The rule, per molecule, over ALL its atoms (the components are ranked together):
 * Initial key of atom a: the pair, compared in this order, of
 *   1. the bytes mnx_smiles_pack writes for the atom (no mark: C, [nH], [13CH3], [O-], *, [2*], ...), compared as unsigned bytes,
 *      a prefix in front of the longer string — so every pseudo-atom written '*' has one key: the rank sees what the string shows;
 *   2. the number of bond records at a.
 * Rank: r(a) = the number of atoms of the molecule whose key is strictly smaller. Equal keys get equal ranks; a class of k atoms
 *   with rank v leaves v+1 .. v+k-1 unused.
 * One refinement round: the key of a becomes r(a) followed by the list of the pairs (r(n), c) over a's bond records (n the other
 *   end), the list sorted ascending and compared lexicographically; c is the written bond class: 0 single (`type` 1, 5, 6),
 *   1 double, 2 triple, 3 aromatic, 4 any other. Ranks are taken anew from these keys. Rounds are repeated while a round raises
 *   the number of distinct ranks.
 * Symmetry class: sym_class(a) = r(a) when the first refinement stops, before any tie is broken. Every automorphism of the
 *   labelled bond graph maps each class onto itself; the converse does not hold (the known limit below).
 * Ties: while two atoms share a rank — take the lowest shared rank v; among its atoms the one with the smallest (x_bin, y_bin,
 *   atom index) keeps v, the others get v+1; refine again. Coordinates come first so that the result does not depend on the
 *   numbering of a given drawing; the index decides only between atoms drawn on the same bin.
 * End state: the ranks are a permutation of 0 .. n_atoms-1.
 * The string: the one mnx_smiles_pack_marks writes for the same drawing with atom a renumbered rank[a] (bond records rewritten
 *   with the lower number as i, `type` and `rev` swapped where the ends swap): its "lowest atom index" and "ascending atom index"
 *   read as "lowest rank" and "ascending rank". order[atom0 + a] is the written position of atom a; n_rings, flag bits 0-12 and
 *   every rule of the marks are those of mnx_smiles_pack_marks on the renumbered molecule, and its strip invariants hold among
 *   the four canonical strings of a molecule. A bond is therefore WRITTEN with the class its lower-ranked end sees (`type` or
 *   `rev`) and RANKED (c above) by the `type` of its record. In the tables of mnx_graph_pack the two have the same written class
 *   (the bond head is symmetrised; a wedge and its mirror are both single); the statements below presume that.
 * Flag bits 13 (MNX_SMILES_CANON_TIE): a tie was broken; 14 (MNX_SMILES_CANON_TIE_INDEX): in some tie the atom that kept v shares
 *   its x_bin and y_bin with another atom of the tie, so the atom index alone decided. Both describe the ranks and are set
 *   wherever the ranks are valid.
 * What follows:
 *   bit 14 clear — the bytes do not change under any renumbering of the atoms or reordering of the bond records of the SAME
 *     drawing, for every `marks`;
 *   bit 13 clear — the marks == 0 bytes depend on the bond graph and the atoms' texts alone;
 *   bit 13 set — the marks == 0 bytes are still the same for every drawing whenever the tied atoms are equivalent under a symmetry
 *     of the graph, the normal case (the oracle of the tests: 0 differing strings over 600 redrawn and renumbered copies of
 *     200 generated molecules);
 *   KNOWN LIMIT — refinement cannot tell some atoms apart that no symmetry exchanges, and then the drawing decides: a six-ring
 *     beside two three-rings in one molecule is written C1CCCCC1.C1CC1.C1CC1 from one drawing and C1CC1.C1CC1.C1CCCCC1 from
 *     another;
 *   under bit 13 the stereo marks ('@', '/', '\') can depend on which of two constitutionally equal atoms the drawing puts first.
 *     No symmetry check of the marks is made here either; mnx_smiles_pack_symmetric below makes one from sym_class.
 * Examples (atoms in index order; bonds (i, j) or (i, j, type)):
 *   O C C, (0,1) (1,2)                          ->  CCO, ranks 2 1 0
 *   [O-] C O C, (0,1,1) (1,2,2) (1,3,1)         ->  CC(=O)[O-]
 *   the alanine of mnx_smiles_pack_stereo       ->  marks 0: C[CH](C(O)=O)N, marks 3: C[C@@H](C(O)=O)N
 *   the F/C=C/F of mnx_smiles_pack_marks        ->  marks 0: C(=CF)F, marks 3: C(=C\F)/F; one tie, classes 2 0 0 2
 *   toluene, the methyl on ring atom 2          ->  Cc1ccccc1
 *   benzene c1ccccc1, naphthalene c1ccc2ccccc2c1, neopentane CC(C)(C)C, cubane C12C3C4C1C1C2C3C41
 *
 * rank: uint16 [n_atom_records], REQUIRED, 2-byte aligned: rank[atom0 + a]. An output, and the only state carried from the first
 *   launch to the others. sym_class: the same shape, or NULL. Both hold 0xFFFF for every atom of a molecule refused on flag bits
 *   0, 1 or 4, exactly where `order` does; a molecule refused on bit 5 (ring numbers) gets no string and keeps valid ranks and
 *   classes. Entries of atoms outside the table, and of no molecule, are not written.
 * Four launches (ranks, count, scan, fill), asynchronous on `stream`, no allocation, no host synchronisation; deterministic
 * word for word (no atomic decides a rank or an order). One workgroup ranks one molecule; the ranks take at most 2 * n_atoms
 * rounds of at most n_atoms^2 / 256 key comparisons per thread. Measured on an MI355X: 1.6 times the time of
 * mnx_smiles_pack_marks on 1024 drug-like molecules (0.47 ms against 0.28 ms), 3 times on near-complete graphs; the worst
 * molecules of 999 atoms hold one workgroup for 0.29 s (identical isolated atoms: 998 ties) and 0.41 s (one ring of 999: about
 * a thousand rounds) — a caller who cannot afford that for a hostile input bounds n_atoms before the call.
 * MNX_ERR_INVALID_ARG as mnx_smiles_pack_marks, and for a null `rank`; the text begins "mnx_smiles_pack_canonical: ". */
#define MNX_SMILES_CANON_TIE 8192u
#define MNX_SMILES_CANON_TIE_INDEX 16384u
int mnx_smiles_pack_canonical(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                              const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes,
                              mnx_smiles* recs, uint16_t* order, uint16_t* rank, uint16_t* sym_class, char* out,
                              uint32_t out_cap, uint32_t* totals, uint32_t marks, void* stream);

/* mnx_smiles_pack_canonical with a SYMMETRY RULE for the marks: a tetrahedral candidate with two substituents of one symmetry
 * class, and a candidate double bond with such a pair at one end, write no mark — so that 2-fluoropropane drawn with a wedge and
 * its mirror image, or (CH3)2C=CHF drawn either way, get ONE string. The arguments, limits, sizing protocol (`totals`), refusal
 * cases and four launches are those of mnx_smiles_pack_canonical, plus `atom_marks`; `marks` is 0..3 as there (any other bit is
 * MNX_ERR_INVALID_ARG). Every older call keeps its bytes, flags and messages. The rule is this library's own; no toolkit has
 * parsed the output.
 *
 * Definitions:
 *   cls(a) is sym_class[a].
 *   A bond is OFF EVERY CYCLE when it lies on no cycle of the molecule's bond graph (the test mnx_smiles_pack_marks makes for
 *     its candidates).
 *   An EQUAL PAIR AT u is two distinct atoms s1, s2, both bonded to u, with cls(s1) == cls(s2) and BOTH bonds u-s1 and u-s2 off
 *     every cycle.
 *   The rule is OFF for a molecule that holds a pseudo-atom (flag bit 2): every pseudo-atom written '*' has one key in the
 *     ranking, so Ph and OMe labels look equal; callers expand first (mnx_expand_pack). Such a molecule gets exactly the bytes
 *     and flags of mnx_smiles_pack_canonical.
 * Tetrahedral (marks bit 0): a candidate centre (the four conditions of mnx_smiles_pack_stereo, unchanged) that has an equal
 *   pair among its explicit neighbours writes NO mark: it is written as the unmarked call writes it, [C] or [CH]. It sets
 *   MNX_ATOM_MARK_SYM at the atom and flag bit 15 (MNX_SMILES_SYM_DROPPED). It does NOT set bit 9 (unresolved); its determinant
 *   is not looked at: symmetry is tested first. Every other candidate follows the old rule unchanged. Bit 6 keeps its own rule —
 *   a wedge neither end of which received a mark — so a wedge at a dropped centre counts.
 * Double bonds (marks bit 1): a candidate is SYMMETRIC when it meets the four unchanged conditions and one of its ends has two
 *   substituents that form an equal pair at that end. A symmetric candidate writes no symbols; it takes no part in the flip rule,
 *   exactly as a bond that is no candidate; it does not set bit 11; it never raises bit 12 (whatever configuration a reader
 *   takes there names the same molecule); it sets MNX_ATOM_EZ_SYM at both ends and flag bit 15. Every other candidate follows
 *   the old rule, taken over the remaining candidates.
 * Invariants:
 *   1. order, rank, sym_class, n_rings and flag bits 0-5, 7, 13 and 14 are those of mnx_smiles_pack_canonical with the same marks.
 *   2. Removing every '@', '/' and '\' from the string gives the marks == 0 canonical bytes (the '-' between two aromatic atoms
 *      put back as stated at mnx_smiles_pack_marks).
 *   3. A molecule with bit 15 clear has the bytes and flags of mnx_smiles_pack_canonical, byte for byte.
 *   4. Bit 13 clear implies bit 15 clear: no two atoms share a class.
 *   5. marks == 0 is mnx_smiles_pack_canonical with marks == 0.
 *   6. The '@' / '@@' that remain stand at the same atoms with the same symbol as in mnx_smiles_pack_canonical: the two
 *      tetrahedral rules never look at each other.
 *   7. There is NO such subset invariant for '/' and '\': removing a symmetric candidate from a conjugated chain can change the
 *      flip of a later one.
 * Examples (atoms with (x_bin, y_bin), bonds (i, j, type, rev); "mirrored" = the same with y replaced by its mirror image):
 *   F(20,30) [C@H](20,20) C(11,15) C(29,15), (0,1,6,5) (1,2,1,1) (1,3,1,1)
 *       canonical marks 3: C[C@@H](C)F, mirrored C[C@H](C)F   ->  C[CH](C)F for both; bits 15 and 6 set, 8 and 9 clear
 *   F(20,30) [C@@](20,20) Cl(20,10) C(11,25) C(29,25) C(3,20) C(37,20), (0,1,6,5) (1,2,1,1) (1,3,1,1) (1,4,1,1) (3,5,1,1)
 *   (4,6,1,1)   canonical: CC[C@@](CC)(Cl)F, mirrored CC[C@](CC)(Cl)F                ->  CC[C](CC)(Cl)F for both
 *   [C@](20,20) C(30,26) C(30,14) C(10,14) C(10,26), (0,1,1,1) (0,2,1,1) (1,2,1,1) (0,3,5,6) (0,4,1,1)
 *       canonical: C[C@@]1(C)CC1, mirrored C[C@]1(C)CC1      ->  C[C]1(C)CC1: the methyls are the equal pair, the ring neighbours
 *       are not off a cycle
 *   the alanine of mnx_smiles_pack_stereo (all classes distinct)                     ->  C[C@@H](C(O)=O)N, unchanged, bit 15 clear
 *   cis- / trans-1,4-dimethylcyclohexane: [C@H](10,20) C(15,11) C(25,11) [C@H](30,20) C(25,29) C(15,29) C(0,20) C(40,20),
 *   (0,1,1,1) (1,2,1,1) (2,3,1,1) (3,4,1,1) (4,5,1,1) (0,5,1,1) (0,6,5,6) and (3,7,5,6) or (3,7,6,5)
 *       ->  KEPT: C[C@H]1CC[C@@H](C)CC1 (cis) and C[C@H]1CC[C@H](C)CC1 (trans); the ring neighbours share a class, but their
 *       bonds lie on the ring
 *   C(0,0) C(0,20) C(10,10) C(20,10) F(30,0), (0,2,1,1) (1,2,1,1) (2,3,2,2) (3,4,1,1)
 *       canonical marks 2: C/C(/C)=C\F, mirrored C/C(/C)=C/F  ->  CC(C)=CF for both; bit 15 set, 10 and 11 clear
 *   F(0,0) F(0,20) C(10,10) C(20,10) F(30,0) F(30,20), (0,2,1,1) (1,2,1,1) (2,3,2,2) (3,4,1,1) (3,5,1,1)
 *       canonical: C(=C(/F)\F)(/F)\F                          ->  C(=C(F)F)(F)F
 *   C(0,20) C(10,10) C(20,20) C(30,10) C(40,20) C(50,20) C(40,30), (0,1,1,1) (1,2,2,2) (2,3,1,1) (3,4,2,2) (4,5,1,1) (4,6,1,1)
 *       canonical: C/C=C/C=C(\C)/C   ->  C/C=C/C=C(C)C: bits 15 and 10 set, 12 clear; the first double bond keeps its marks
 *   the F/C=C/F of mnx_smiles_pack_marks                       ->  C(=C\F)/F, unchanged: each end has one substituent
 * KNOWN LIMITS:
 *   the ranks ignore stereo: a pseudo-asymmetric centre, whose two branches differ only by their own marks, is dropped;
 *   a pair on ring bonds is never dropped: a cyclohexylidene end and a spiro centre keep spurious marks;
 *   the ring cis/trans and meso cases can still depend on which of two tied atoms the drawing puts first: the bit 13 sentence of
 *     mnx_smiles_pack_canonical stays true for those;
 *   refinement's known limit carries over: classes can be equal although no symmetry exchanges the atoms, and then a true
 *     centre is dropped;
 *   an explicit [H] neighbour is an atom like any other and is not equated with the implicit H.
 *
 * rank AND sym_class: both REQUIRED here (the class is state between the rank launch and the writers; the call allocates
 *   nothing). atom_marks: uint8 [n_atom_records] or NULL: the MNX_ATOM_* bits of atom0 + a, and 0xFF for every atom of a molecule
 *   to which `order` gives 0xFFFF; entries outside every molecule are not written. Four launches, asynchronous on `stream`,
 *   deterministic word for word. Measured on an MI355X against mnx_smiles_pack_canonical on 1024 drug-like molecules: the same
 *   time at marks 0, 2 and 3 (inside the runs' spread), 5 % more at marks 1 (0.51 ms against 0.49 ms: the off-every-cycle pass,
 *   which only the double-bond stage ran before). MNX_ERR_INVALID_ARG as mnx_smiles_pack_canonical, and for a null `sym_class`;
 *   the text begins "mnx_smiles_pack_symmetric: ". */
#define MNX_SMILES_SYM_DROPPED 32768u        /* flag bit 15 */
#define MNX_ATOM_MARK_CW 1u                  /* '@' written at this atom */
#define MNX_ATOM_MARK_CCW 2u                 /* '@@' written */
#define MNX_ATOM_MARK_SYM 4u                 /* tetrahedral candidate, dropped: an equal pair */
#define MNX_ATOM_EZ 8u                       /* end of a double bond that got '/' '\' */
#define MNX_ATOM_EZ_SYM 16u                  /* end of a candidate double bond dropped for symmetry */
int mnx_smiles_pack_symmetric(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                              const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes,
                              mnx_smiles* recs, uint16_t* order, uint16_t* rank, uint16_t* sym_class, uint8_t* atom_marks,
                              char* out, uint32_t out_cap, uint32_t* totals, uint32_t marks, void* stream);

/* The fragments that abbreviation labels stand for, for mnx_expand_pack: a label such as 'Ph', 'OMe' or 'Boc' that the tokenizer
 * emits as ONE atom, as the atoms and bonds it means. The library is data of the caller (molnextr_amd/vocab/fragments.json, written
 * from what each name means chemically; NOT the reference's abbrs.py), handed over as packed tables of the record types of
 * mnx_graph_pack: one mnx_mol record is one fragment, with its mnx_atom / mnx_bond records and a text arena of the atom symbols.
 * Atom 0 of a fragment is the attachment atom: every bond of the label goes to it. Of a fragment record atom0, n_atoms, bond0,
 * n_bonds, text0 and smiles_len are read (smiles_len only to test that the text lies inside `text`); of an atom sym0 and sym_len;
 * of a bond i, j, type and rev. frag_of_name [n_names] is parallel to the names of mnx_set_symbol_tables: the fragment of name k,
 * or -1. The lookup of an atom's symbol therefore is the writers' own lookup in those names: "is an abbreviation" and "has a
 * fragment" cannot drift apart. Host pointers, validated and copied to the device before the call returns (one allocation, sized
 * here, freed by mnx_destroy or by the next call; a fragment's bonds are sorted by (i, j) in that copy): a sibling of
 * mnx_set_symbol_tables, which must have been called, and which drops the fragments when it is called again.
 * The caller vouches for one thing the library does not test: every fragment atom's symbol is an atom of the SMILES grammar
 * under the interpretation of mnx_molfile_pack and no name of the tables (molnextr_amd/fragments.py tests it).
 * MNX_ERR_INVALID_ARG (with mnx_last_error, "mnx_set_fragments: ..."), nothing is copied or launched then: no symbol tables set;
 * n_frags outside 0..512; n_names not the n of mnx_set_symbol_tables; a null pointer (a table of size 0 may be null); a fragment
 * of 0 or more than 32 atoms; records that end behind a table; a symbol of 0 or more than 8 bytes or one that ends behind the
 * text; a bond without i < j < n_atoms, with a type outside 1..4 or with rev != type; the same pair of atoms in two bonds;
 * frag_of_name[k] outside -1..n_frags-1, or >= 0 for a name that is not of kind 2. */
int mnx_set_fragments(mnx_engine* h, const mnx_mol* frags, int32_t n_frags, const mnx_atom* atoms, uint32_t na,
                      const mnx_bond* bonds, uint32_t nb, const char* text, uint32_t nt, const int32_t* frag_of_name,
                      int32_t n_names);

/* Abbreviation labels replaced by their atoms and bonds, on the device: packed tables of mnx_graph_pack in, packed tables of the
 * SAME record types out, so that mnx_molfile_pack and the four mnx_smiles_pack calls run on the expanded molecule unchanged — a
 * label on one drawing and the drawn-out group on another then get the same canonical string. What the reference's
 * _expand_functional_group does for an alias that is a key of its table; from a table only: a condensed formula ('CH2CH3',
 * 'N(CH3)2') is mnx_formula_pack's, in front of this call, and the reference's fragments of zero atoms ('H3', '(H)': delete the
 * atom) are out of scope, such a label stays. No toolkit has parsed or sanitised the result. A post-pass on a post-pass: it reads the input
 * tables, changes none of them (the outputs must not overlap them) and touches no decode state.
 *
 * Which atoms expand: an atom whose symbol, read as mnx_molfile_pack reads it (one pair of enclosing '[' ']' stripped, the
 * R-group table first, then the abbreviation table), is an abbreviation (kind 2) whose frag_of_name is >= 0. R-groups, symbols
 * without a parse and abbreviations without a fragment never expand.
 * Atoms: the molecule's n_atoms atoms keep their indices. A label at index i becomes atom 0 of its fragment, still at index i.
 * Fragment atoms 1..m-1 are appended behind the molecule's own atoms, labels in ascending index, fragment atoms in ascending
 * order. Every atom of a fragment, the one at i included, takes the label's index, x_bin, y_bin and score: the coordinates
 * COINCIDE inside a fragment — a 2D layout of fragments is out of scope (a molfile of the result is a connection table, not a
 * drawing; the double-bond marks of mnx_smiles_pack_marks find nothing to resolve inside a fragment).
 * Bonds: every bond record of the input is kept with its i, j, type, rev and score — a bond of the label goes to the attachment
 * atom. Every fragment bond is added with its ends mapped to the new indices, rev = type and the score of the label atom. The
 * table keeps the documented order, i ascending, then j ascending: row i holds the input's records of row i in their order and
 * behind them, for a label, the fragment's bonds from the attachment atom by ascending j; the rows of the appended atoms hold the
 * fragment's other bonds.
 * Text: the text of an output molecule is its atoms' symbols behind one another in the order of the new indices, smiles_len its
 * length. It is NO LONGER a token SMILES; mnx_atom.sym0 is a span of it as before.
 * origin uint16 [atom_cap] (may be null): origin[atom0 + k] = the input index of the atom that output atom k came from — k itself
 * for k < n_atoms of the input, the label's index for an appended atom.
 * mnx_mol.flags of the output: bit 0 is copied; MNX_MOL_EXPANDED: at least one label was replaced; MNX_MOL_LABEL_LEFT: a
 * pseudo-atom other than a parsed '*' remains (an R-group, an abbreviation without a fragment, a symbol without a parse);
 * MNX_MOL_EXPAND_REFUSED: the molecule's records point beyond the tables passed — the test of MNX_MOLFILE_BEYOND_TABLES: atom0 +
 * n_atoms, bond0 + n_bonds or text0 + smiles_len beyond the sizes passed, a symbol beyond n_text_bytes, a bond whose i or j is no
 * atom of the molecule —, or its bond records are not sorted by i (a record's i below its predecessor's: the place of a label's
 * bonds is found by a search in them; mnx_graph_pack writes them sorted), or it has more than 2047 atoms (2047 x 32 atoms always
 * fit the uint16 indices), or more than 2^32 - 1 bonds afterwards. A refused molecule has n_atoms = n_bonds = smiles_len = 0 in
 * mols_out. overall_score is copied.
 * Inputs as mnx_molfile_pack's: mols [n], 1 <= n <= 65536; atoms [n_atom_records], bonds [n_bond_records] (8-byte aligned),
 * text [n_text_bytes]. mnx_set_symbol_tables and mnx_set_fragments must have been called.
 * Outputs, device pointers the caller allocated, as mnx_graph_pack's: mols_out [n]; atoms_out [atom_cap], bonds_out [bond_cap]
 * (8-byte aligned), text_out [text_cap] bytes; totals uint32 [4] = {atoms, bonds, text bytes needed, 1 if any capacity was too
 * small}. When a capacity is too small nothing is written beyond it (origin follows atom_cap), and mols_out and totals are
 * complete all the same: read the needed sizes and call again. Deterministic word for word (every position comes from a prefix
 * scan or a search in sorted records; no atomics); records are written whole, padding bytes as zeros. Three launches,
 * asynchronous on `stream`, no allocation, no host synchronisation.
 * MNX_ERR_INVALID_ARG (with mnx_last_error, "mnx_expand_pack: ..."): a null pointer (a table with capacity 0 may be null), n
 * outside 1..65536, misaligned records, or no symbol tables / fragments set; nothing is launched then. */
#define MNX_MOL_EXPANDED 2u
#define MNX_MOL_LABEL_LEFT 4u
#define MNX_MOL_EXPAND_REFUSED 8u
int mnx_expand_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                    const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_mol* mols_out,
                    mnx_atom* atoms_out, uint32_t atom_cap, mnx_bond* bonds_out, uint32_t bond_cap, char* text_out,
                    uint32_t text_cap, uint16_t* origin, uint32_t* totals, void* stream);

/* Condensed-formula labels replaced by the atoms and bonds they spell, on the device: packed tables in, packed tables of the SAME
 * record types out. mnx_expand_pack replaces a label only when its name has a fragment; every other label the tokenizer can spell
 * character by character ('CH2CH3', 'N(CH3)2', 'COOCH3', 'SO2CH3', 'CH2Ph', '(CH2)2OH') is this call's. Intended order:
 * mnx_graph_pack or mnx_smiles_read -> THIS CALL -> mnx_expand_pack -> mnx_kekulize_pack -> mnx_normalize_pack -> the writers.
 * THE RULE IS THIS LIBRARY'S OWN: it keeps the shape of the reference's valence-guided search (get_smiles_from_symbol: placement
 * order, branch-or-chain decision, direction retry) and repairs it so that its result is a molecule — hydrogens are counted,
 * no bond above order 3, no bonds left over at the end, a step limit. No toolkit has parsed the result. A post-pass on a post-pass:
 * it reads the input tables, changes none of them (the outputs must not overlap them) and touches no decode state.
 *
 * Candidates: an atom whose symbol, read as mnx_molfile_pack reads it, has no parse as an atom of the grammar, is in neither
 *   symbol table, and has 2 to 20 bytes after one pair of enclosing '[' ']' is stripped. R-groups and table names never come
 *   here, with or without a fragment. A candidate with a bond record of class 4 (aromatic), or of a type outside 1, 2, 3, 5, 6,
 *   stays a label.
 * Tokens, left to right: '(' , ')' and a run of digits (a count, 1..99). At an upper-case byte the maximal run [A-Z][a-z]*: if it
 *   is an element of the valence table, that element; otherwise the longest name of the abbreviation table that HAS a fragment
 *   (frag_of_name >= 0) and matches at this position is a group token. At a lower-case byte only such a name matches ('tBu' in
 *   'CO2tBu'). Any other byte ('=', '#', '+', '-', ',', ...): the label stays.
 * Valences, in the order of trial: H 1; B 3; C 4; N 3, 5; O 2; F, Cl, Br, I 1; Si 4; P 5, 3; S 6, 4, 2. A group token has
 *   valence 1. P and S try the highest first: the condensed formulas that occur (SO2, PO3, SO2NH2) mean that state, and the end
 *   condition rejects it where it is wrong (SH, SCH3).
 * Units: an element, a group token or a parenthesised sequence (not empty, nesting depth at most 3), each with an optional count
 *   behind it; a count anywhere else: the label stays. Counts are written out: a unit with count k is k units, but 'Hk' is ONE
 *   unit of k hydrogens. 'C' with a count n > 1 directly followed by an element X with count m is n times C, each followed by
 *   m / n X, the remainder behind the last: C2H5 = CH2CH3. More than 96 units and parentheses, or more than 32 heavy atoms and
 *   group tokens, written out: the label stays.
 * The search: start = the bond-order sum of the label's bond records (types 1, 5, 6 count 1; 2 and 3 their order); above 6 the
 *   label stays. Direction 1 places the units from left to right; if that finds no structure, direction -1 places them from
 *   right to left (every parenthesis turned round). Units are placed in order onto a CURRENT atom with `free` bonds:
 *   - The first heavy atom or group token of the label takes the label's bonds: it needs a valence v >= start, becomes the current
 *     atom, free = v - start.
 *   - A heavy atom or group token of valence v, with free >= 1: if free > v it is a leaf on a bond of order v and free -= v;
 *     otherwise its bond has order `free`, it becomes the current atom, and free = v - free. free == 0: the branch fails.
 *   - k hydrogens need free >= k and are recorded as the H COUNT of the current atom, free -= k; they are never atoms, and
 *     without a current atom (first of the label or of a branch) the branch fails.
 *   - '(' with a current atom that has more than 1 bond free opens a BRANCH: its first heavy atom hangs on the current atom
 *     (valence >= 1, free = v - 1) and the units up to its ')' are placed onto it and its successors. At the ')' the bonds left
 *     free raise the order of the joining bond to 1 + left, the current atom is the one in front of the '(' again, and its free
 *     bonds are reduced by that order: C(O)CH3 is C(=O)C. Left-over bonds beyond those of the current atom fail the branch.
 *     Any other '(' (1 bond free, or no current atom yet) and its ')' change nothing: the group continues the chain. 0 bonds
 *     free: the branch fails.
 *   - A bond order above 3 fails the branch.
 *   - The end of the label needs free == 0: every hydrogen of a condensed formula is written, nothing is inferred.
 *   - Valences are tried in table order with backtracking through the whole label (depth first; the last element placed that
 *     has another valence tries it next).
 *   - Every placement of a heavy atom, a group token or a unit of hydrogens is a step, counted over both directions; beyond
 *     max_steps (0: MNX_FORMULA_DEFAULT_STEPS) the label stays and MNX_MOL_FORMULA_LIMIT is set.
 * Output: exactly mnx_expand_pack's rule for atoms, bonds, text and origin, with the searched structure in the place of the
 *   table's fragment: atom 0 is the first placed atom and stays at the label's index, the others are appended behind the
 *   molecule's own atoms in placement order, labels in ascending index; all atoms of a structure share the label's index,
 *   coordinates and score; the structure's bonds have rev = type and the label atom's score, the rows sorted by (i, j) as there.
 *   A heavy atom is spelled unbracketed when it is of B C N O P S F Cl Br I and a reader infers its H count from its bond-order
 *   sum (the smallest normal valence that fits, as mnx_normalize_pack), else as a bracket atom with its H count: CH2CH3 writes
 *   'C', 'C' — the bytes the table's Et gives —, Si(CH3)3 writes '[Si]', 'C', 'C', 'C'. A group token is written as '[Name]', so
 *   that the following mnx_expand_pack expands it.
 * mnx_mol.flags of the output: bit 0 is copied; MNX_MOL_FORMULA_EXPANDED: at least one label was replaced;
 *   MNX_MOL_FORMULA_LEFT: a candidate stayed (no tokenisation, no structure, too large, a bond that is no bond order, the step
 *   limit); MNX_MOL_FORMULA_LIMIT: the search of a label passed the step limit; MNX_MOL_FORMULA_REFUSED: the refusal conditions
 *   of MNX_MOL_EXPAND_REFUSED. A refused molecule has n_atoms = n_bonds = smiles_len = 0 in mols_out. overall_score is copied.
 * What it is not: a two-ended label ('CH2CH2' between two atoms) keeps all its bonds on atom 0 and usually finds no structure —
 *   that would need the drawing's left and right; rings (C6H5, C6H11), explicit bond symbols, charges and isotopes ('D' included)
 *   are refused; PO3H2 finds no structure, because the chain rule gives the second O the last bonds; where several structures are
 *   valid the valence order decides.
 * Inputs, outputs, the capacity / totals protocol, determinism and the launches (three, asynchronous on `stream`, no allocation, no
 * host synchronisation) are mnx_expand_pack's. mnx_set_symbol_tables and mnx_set_fragments must have been called.
 * MNX_ERR_INVALID_ARG (with mnx_last_error, "mnx_formula_pack: ..."): a null pointer (a table with capacity 0 may be null), n
 * outside 1..65536, misaligned records, or no symbol tables / fragments set; nothing is launched then. */
#define MNX_MOL_FORMULA_EXPANDED 1024u
#define MNX_MOL_FORMULA_LEFT 2048u
#define MNX_MOL_FORMULA_LIMIT 65536u
#define MNX_MOL_FORMULA_REFUSED 131072u
#define MNX_FORMULA_DEFAULT_STEPS 4096u
int mnx_formula_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                     const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_mol* mols_out,
                     mnx_atom* atoms_out, uint32_t atom_cap, mnx_bond* bonds_out, uint32_t bond_cap, char* text_out,
                     uint32_t text_cap, uint16_t* origin, uint32_t* totals, uint32_t max_steps, void* stream);

/* The main molecule of every molecule, on the device: packed tables in, packed tables of the SAME record types out, with the
 * connected component that has the most atoms kept and every other atom and its bonds dropped — salts, counter-ions, solvent and
 * the stray atoms a bond head leaves unconnected. Intended order: mnx_graph_pack or mnx_smiles_read -> mnx_formula_pack ->
 * mnx_expand_pack -> THIS CALL -> mnx_kekulize_pack -> mnx_normalize_pack -> the writers: behind the expansion, so that a label
 * counts with the atoms it stands for, as the reference counts them after _expand_functional_group ('[Ph].CCCCC' keeps the ring
 * behind mnx_expand_pack and the chain in front of it).
 * THE RULE IS THE REFERENCE'S (_keep_main_molecule: GetMolFrags, np.argmax of the sizes): it is graph connectivity and a maximum
 * and needs no toolkit to state. A component is a set of atoms joined by bond records; every record joins its ends whatever its
 * type, a record with i == j joins nothing, the same pair in several records counts once. The size of a component is the number
 * of its atom records (hydrogens that a symbol implies are no atoms). The component with the most atoms stays; among components of
 * that size the one that holds the lowest atom index stays, as the reference's first of the largest does. A post-pass on a
 * post-pass: it reads the input tables, changes none of them (the outputs must not overlap them) and touches no decode state.
 *
 * Atoms: the kept atoms in ascending input index, renumbered from 0; index, x_bin, y_bin and score are copied.
 * Bonds: a record is kept iff its i is kept (its j is then kept too), in the input's order, i and j mapped to the new indices;
 * type, rev and score are copied. The records need not be sorted; a table sorted by (i, j) stays sorted.
 * Text: the text of an output molecule is the kept atoms' symbols behind one another in the order of the new indices, smiles_len
 * its length, as mnx_expand_pack leaves it — also for a molecule of one component or none, which keeps every atom: the output
 * has one form. mnx_atom.sym0 is a span of it as before. The symbols are copied, not read: no symbol tables are needed.
 * origin uint16 [atom_cap] (may be null): origin[atom0 + k] = the input index of output atom k.
 * mnx_mol.flags of the output: bit 0 is copied, the bits of the other passes are not; MNX_MOL_MAIN_KEPT: the molecule had more
 * than one component and atoms were dropped; MNX_MOL_MAIN_TIE: another component had as many atoms as the kept one, so the choice
 * rests on the numbering of the atoms, as the reference's does; MNX_MOL_MAIN_REFUSED: the molecule's records point beyond the
 * tables passed — atom0 + n_atoms, bond0 + n_bonds or text0 + smiles_len beyond the sizes passed, a symbol beyond n_text_bytes, a
 * bond whose i or j is no atom of the molecule —, or it has more than 2047 atoms (any number of bond records). A refused molecule
 * has n_atoms = n_bonds = smiles_len = 0 in mols_out. overall_score is copied.
 * Inputs and outputs as mnx_expand_pack's, argument for argument: mols [n], 1 <= n <= 65536; atoms [n_atom_records], bonds
 * [n_bond_records] (8-byte aligned), text [n_text_bytes]; mols_out [n]; atoms_out [atom_cap], bonds_out [bond_cap] (8-byte
 * aligned), text_out [text_cap] bytes; totals uint32 [4] = {atoms, bonds, text bytes needed, 1 if any capacity was too small}.
 * Nothing grows: the input's sizes always suffice. When a capacity is too small nothing is written beyond it (origin follows
 * atom_cap), and mols_out and totals are complete all the same: read the needed sizes and call again. Deterministic word for word:
 * every position comes from a prefix scan; the components come from integer minima, sums and one maximum in on-chip memory, whose
 * results do not depend on the order they are taken in. Records are written whole, padding bytes as zeros. Three launches,
 * asynchronous on `stream`, no allocation, no host synchronisation.
 * MNX_ERR_INVALID_ARG (with mnx_last_error, "mnx_main_pack: ..."): a null pointer (a table with capacity 0 may be null), n outside
 * 1..65536, or misaligned records; nothing is launched then. */
#define MNX_MOL_MAIN_KEPT 262144u
#define MNX_MOL_MAIN_TIE 524288u
#define MNX_MOL_MAIN_REFUSED 1048576u
int mnx_main_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                  const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_mol* mols_out,
                  mnx_atom* atoms_out, uint32_t atom_cap, mnx_bond* bonds_out, uint32_t bond_cap, char* text_out,
                  uint32_t text_cap, uint16_t* origin, uint32_t* totals, void* stream);

/* One normal spelling per atom, on the device: packed tables in, packed tables of the SAME record types out, with aromatic rings
 * perceived from Kekule drawings, hydrogens counted and brackets dropped where a reader infers what they say. The canonical ranks key
 * on the bytes a writer puts down for an atom, so without this pass c1ccccc1 never equals C1=CC=CC=C1, C[CH](C)F never equals
 * CC(C)F, and a pyrrole drawn with N never equals [nH]. Intended order: mnx_smiles_read or mnx_graph_pack -> mnx_expand_pack ->
 * THIS CALL -> mnx_molfile_pack / the mnx_smiles_pack calls, all of which run on the output unchanged.
 * THE RULE IS THIS LIBRARY'S OWN. It is NOT RDKit's aromaticity model (nor Daylight's, nor any toolkit's), no toolkit has checked
 * it, and a string written behind it never compares with a toolkit's. It only goes from Kekule to aromatic: the other direction is
 * mnx_kekulize_pack's, below.
 * A post-pass on a post-pass: it reads the input tables, changes none of them (the outputs must not overlap them) and touches no
 * decode state. Atom and bond COUNTS and ORDER never change: only the text, an atom's sym0 / sym_len and a bond's type / rev do.
 *
 * The rule, per molecule:
 * Interpretation. Every atom's symbol is read as mnx_molfile_pack reads it. COPIED, byte for byte, taking part in nothing below:
 *   a pseudo-atom (R-group, abbreviation, a symbol without a parse), a parsed '*' with or without brackets, an atom whose element
 *   is spelled in lower case already, and an EXCLUDED atom (next paragraph). The four chiral carbon symbols [C@] [C@@] [C@H]
 *   [C@@H] are interpreted (their H count is the written one) but never candidates, and their bytes are copied too, so that
 *   mnx_smiles_pack_stereo still finds its centres. Every other atom is INTERPRETED: (isotope, element, H, charge).
 * Bonds. By `type` (rev is not read): 1, 5 and 6 are single (order 1), 2 double, 3 triple. An atom with a bond record of type 4
 *   or of any other type, or with a record from the atom to itself, is EXCLUDED. So every bond of an atom that is not excluded has
 *   an integer order; bo(a) is the sum of the orders of the bond records at a, deg(a) their number.
 * Hydrogens H(a). A bracket atom has its written count. An unbracketed atom of the organic subset has v - bo(a) for the smallest
 *   normal valence v >= bo(a), 0 when there is none: B 3; C 4; N 3, 5; O 2; P 3, 5; S 2, 4, 6; F, Cl, Br, I 1.
 * Candidates. An interpreted C, N, O or S that is none of the chiral symbols, with deg <= 3, all its bond records to different
 *   atoms, no triple bond, and one of
 *     (d) exactly one double bond, and it is C with charge 0 or N with charge 0 or +1;
 *     (p) no double bond, and it is N with charge 0 and deg + H = 3, or O or S with charge 0, deg = 2 and H = 0, or C with
 *         charge -1 and deg + H = 3;
 *     (e) no double bond, and it is C with charge +1.
 * Rings. The ENUMERATED rings are the simple cycles of exactly 5 or 6 atoms that are all candidates (their bonds are single or
 *   double by the above). A bond on an enumerated ring is a RING-SYSTEM bond. Which rings are enumerated does not depend on any
 *   verdict, so no fixed point is iterated: the ring-system bonds are marked first, then every ring is judged.
 * Electrons of atom a in ring R: (p) 2; (e) 0; (d) 1 when a's double bond is a ring-system bond (in R or in a fused enumerated
 *   ring); (d) 0 when a is C and its double bond goes to an O, N or S atom (any spelling that parses) that lies on no enumerated
 *   ring — the exocyclic C=O of a pyridone; in every other case R FAILS. R is AROMATIC when it does not fail and the sum is 6.
 * Marking. Every atom of an aromatic ring becomes lower case; every bond of an aromatic ring gets type = rev = 4 (a wedge there
 *   is lost). Every other bond record keeps its fields: the writers put '-' between two aromatic atoms joined by a single bond.
 * Spelling of an interpreted atom, from (isotope, element, aromatic, H, charge): WITHOUT brackets when the element is of the
 *   organic subset, there is no isotope, the charge is 0 and H is what a reader infers — for an upper-case atom the valence
 *   table above on bo(a) (an upper-case atom has none of the new aromatic bonds, so bo is the same on the output), for a new c
 *   3 - deg, for a new n, o, s 0. Otherwise a bracket atom exactly as mnx_smiles_pack spells one: '[', isotope, element, 'H' and
 *   a count above 1, the sign and a count above 1, ']'; 12 bytes at most. An atom class ([C:12]) is dropped, as the writers drop it.
 * Examples (strings as mnx_smiles_read reads and mnx_smiles_pack writes them): C1=CC=CC=C1 -> c1ccccc1. N1C=CC=C1 -> [nH]1cccc1.
 *   CN1C=CC=C1 -> Cn1cccc1. C1=CN=CN1 -> c1cnc[nH]1. O=C1C=CC=CN1 -> O=c1cccc[nH]1. [CH-]1C=CC=C1 -> [cH-]1cccc1. Both Kekule
 *   forms of naphthalene -> c1ccc2ccccc2c1 (the fused atoms count their double bond in the other ring). C1=CC=CC=C1C1=CC=CC=C1 ->
 *   c1ccccc1-c1ccccc1. NOT aromatic: C1=CC=CCC1, C1=CC=CC1 (a CH2 is no candidate), O=C1C=CC(=O)C=C1 (4 electrons), C=C1C=CC=C1
 *   (the exocyclic double bond goes to C). Brackets: C[CH](C)F -> CC(C)F, [CH3][CH2][OH] -> CCO; [CH2]C, [13CH4], [NH4+], [C] and
 *   [C@H] stay. The de-marked [CH] that mnx_smiles_pack_symmetric writes is normalised only when that string is read back in.
 * KNOWN LIMITS:
 *   only rings of 5 and 6 atoms are examined: azulene, tropylium and cyclooctatetraene dianion stay Kekule;
 *   a ring that holds a lower-case atom or a class-4 bond is not examined: a half-aromatic fused prediction stays as it came;
 *   this call never kekulises: an aromatic input stays as it came. mnx_kekulize_pack in front of this call gives a half-aromatic
 *     molecule, and an aromatic ring this rule cannot find (azulene), one form;
 *   an explicit [H] atom is an atom like any other and is not folded into a count;
 *   the output is a fixed point of the call on everything tested (a second call changes no table), with one corner that is known
 *     and was not met: a C whose exocyclic double bond goes to an N on a fused enumerated ring that fails while it holds an atom of
 *     an aromatic ring counts 1 the first time and 0 the second, when that fused ring is no longer enumerated;
 *   the H count noted for a copied atom is its written one: an atom this call wrote as a plain c notes 0 when it is copied later.
 *
 * Output. mols_out[b]: n_atoms and n_bonds of the input, smiles_len the length of the new text, which is the atoms' new symbols
 * behind one another in atom order (as mnx_expand_pack's: NO token SMILES); flags = bit 0 copied | MNX_MOL_AROMATIZED (an atom
 * became aromatic) | MNX_MOL_UNBRACKETED (a bracket atom lost its brackets); the MNX_MOL_EXPAND* bits of the input are not
 * copied. An atom record keeps index, x_bin, y_bin and score; a bond record i, j and score; overall_score is copied.
 * MNX_MOL_NORMALIZE_REFUSED: the molecule's records point beyond the tables passed (atom0 + n_atoms, bond0 + n_bonds or text0 +
 * smiles_len beyond the sizes passed, a symbol beyond n_text_bytes, a bond whose i or j is no atom of the molecule), or it has
 * more than 999 atoms or bonds (the writers' limit). A refused molecule has n_atoms = n_bonds = smiles_len = 0 in mols_out.
 * atom_notes uint8 [atom_cap] (may be null): for output atom atom0 + k, bits 0-3 its H count (written for a bracket atom,
 * inferred otherwise; 0 for a copied atom that is no bracket atom), MNX_NOTE_AROMATIZED: made aromatic by this call,
 * MNX_NOTE_UNBRACKETED: its brackets were removed, MNX_NOTE_COPIED: the symbol was copied uninterpreted.
 * Inputs as mnx_expand_pack's: mols [n], 1 <= n <= 65536; atoms [n_atom_records], bonds [n_bond_records] (8-byte aligned), text
 * [n_text_bytes]. mnx_set_symbol_tables must have been called. Outputs, device pointers the caller allocated, with the sizing
 * protocol of mnx_expand_pack: totals uint32 [4] = {atoms, bonds, text bytes needed, 1 if any capacity was too small}; when a
 * capacity is too small nothing is written beyond it (atom_notes follows atom_cap), and mols_out and totals are complete all the
 * same. Deterministic word for word: every position comes from a prefix scan, and the atomics of the kernel only count, add up
 * and set bits of sets. Records are written whole, padding bytes as zeros. Three launches, asynchronous on `stream`, no
 * allocation, no host synchronisation.
 * MNX_ERR_INVALID_ARG (with mnx_last_error, "mnx_normalize_pack: ..."): a null pointer (a table with capacity 0 may be null), n
 * outside 1..65536, misaligned records, or no symbol tables set; nothing is launched then. */
#define MNX_MOL_AROMATIZED 16u
#define MNX_MOL_UNBRACKETED 32u
#define MNX_MOL_NORMALIZE_REFUSED 64u
#define MNX_NOTE_H_MASK 15u
#define MNX_NOTE_AROMATIZED 16u
#define MNX_NOTE_UNBRACKETED 32u
#define MNX_NOTE_COPIED 64u
int mnx_normalize_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                       const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_mol* mols_out,
                       mnx_atom* atoms_out, uint32_t atom_cap, mnx_bond* bonds_out, uint32_t bond_cap, char* text_out,
                       uint32_t text_cap, uint8_t* atom_notes, uint32_t* totals, void* stream);

/* Kekule structures for the aromatic systems of the packed molecule tables, on the device: the inverse of what
 * mnx_normalize_pack perceives. Lower-case atoms on type-4 bonds — as mnx_smiles_read reads c1ccccc1, as the bond head predicts an
 * aromatic ring, as mnx_normalize_pack writes one — become upper-case atoms on double and single bonds, so that a molfile carries
 * no bond type 4 (which the CTfile format keeps for queries) and a molecule has a form that does not depend on which rings a
 * perception rule finds. Packed tables in, packed tables of the same record types out. The intended order is mnx_smiles_read /
 * mnx_graph_pack -> mnx_expand_pack -> THIS CALL -> mnx_normalize_pack (optional) -> the writers.
 * A Kekule structure is a perfect matching of the atoms that must take a double bond, so whether an output is valid can be checked
 * without a toolkit. ONLY THE CHOICE AMONG SEVERAL VALID MATCHINGS IS THIS LIBRARY'S OWN, fixed by the search order below. The rule
 * is NOT RDKit's Kekulize (nor any toolkit's) and no toolkit has checked it.
 * A post-pass on a post-pass: it reads the input tables, changes none of them (the outputs must not overlap them) and touches no
 * decode state. Atom and bond COUNTS and ORDER never change: only the text, sym0 / sym_len of the atoms of kekulised systems and
 * type / rev of their type-4 bond records do.
 *
 * The rule, per molecule:
 * Interpretation. Every atom's symbol is read as mnx_molfile_pack reads it. An AROMATIC ATOM is an interpreted atom whose element
 *   is spelled in lower case (the reader accepts b c n o p s, and se and as in brackets). Everything else — upper-case atoms,
 *   pseudo-atoms, '*', symbols without a parse — is copied byte for byte and is no aromatic atom.
 * Bond orders. By `type` (rev is not read): 1, 5, 6 and 4 count 1, 2 counts 2, 3 counts 3, every other type 0. bo(a) is the sum
 *   over the bond records at a (a record from an atom to itself counts at both of its ends). H(a) is the written count for a
 *   bracket atom, max(0, 3 - bo) for an unbracketed c, and 0 for every other unbracketed lower-case atom.
 * Systems. The vertices are the aromatic atoms, the edges the type-4 records between two aromatic atoms. A SYSTEM is a connected
 *   component; an aromatic atom without a type-4 record is a system of one. A system is BLOCKED, and stays exactly as it came,
 *   when one of its atoms has a type-4 record whose other end is no aromatic atom, or more than three type-4 records, or two
 *   records (of any type) to the same atom or a record to itself, or a record of a type outside 1..6.
 * Needy atoms. v is 4 for c; 3 for b, n, p and as, where a charge of +1 makes n and p 4 and a charge of -1 makes b 4; 2 for o, s
 *   and se, or 3 at charge +1; 3 for c at charge +1 or -1. An atom is NEEDY iff v - bo - H == 1. So pyridine n, the [n+] of an
 *   N-oxide, pyrylium [o+] and an ordinary c are needy; [nH], N-methyl n, o, s, the c(=O) of a pyridone, [cH-] and [cH+] are
 *   not. An (element, charge) pair that is not listed is not needy.
 * Matching, per system, independent of every other system. The edges of the search are the type-4 records between two needy atoms
 *   of the system. An odd number of needy atoms fails at once, and so does a needy atom without a needy neighbour. Otherwise the
 *   search is depth first: take the lowest-index unmatched needy atom and try its unmatched needy neighbours in ascending atom
 *   index; each pairing tried counts one STEP; a pairing is undone at once when it leaves an unmatched needy atom of the system
 *   with no unmatched needy neighbour (only the neighbours of the two atoms just paired can be in that state); when no candidate
 *   is left, backtrack to the previous pairing; backtracking from the first atom fails the system. More than max_steps steps in
 *   one system fails it with the limit bit; max_steps == 0 means MNX_KEKULE_DEFAULT_STEPS. The first complete matching found is
 *   the result. Pruning removes only failing branches, so the result is the lexicographically first matching in that order, and a
 *   search without pruning finds the same one; the step count is defined with the pruning.
 * Writing a system that succeeded. Every atom becomes upper case, spelled by mnx_normalize_pack's spelling rule for an upper-case
 *   atom from (isotope, element, H, charge) and the new bo (one more for a matched atom): without brackets when the element is of
 *   the organic subset, there is no isotope, the charge is 0 and H is what the valence table infers; otherwise a bracket atom
 *   exactly as mnx_smiles_pack spells one. H never changes. Matched records get type = rev = 2, the system's other type-4 records
 *   type = rev = 1; every other record keeps every field. Atoms of systems that failed or were blocked, and all other atoms, are
 *   copied byte for byte.
 * Examples (strings as mnx_smiles_read reads and mnx_smiles_pack writes them): c1ccccc1 -> C1=CC=CC=C1. c1cc[nH]c1 -> C=1C=CNC1 (a
 *   pyrrole with N). O=c1cccc[nH]1 -> O=C1C=CC=CN1. c1ccc2ccccc2c1 -> C1=CC=C2C=CC=CC2=C1. c1ccccc1-c1ccccc1 ->
 *   C1=CC=CC=C1C1=CC=CC=C1 (the link stays single). c1cccc1 is left aromatic, with MNX_MOL_KEKULE_LEFT. [cH-]1cccc1 ->
 *   [CH-]1C=CC=C1. Azulene c1ccc2cccc2cc1 -> C1=CC=C2C=CC=C2C=C1, although mnx_normalize_pack cannot find it.
 * KNOWN LIMITS:
 *   the choice among valid matchings is this library's own order; it is not RDKit's Kekulize and no toolkit has checked it;
 *   that order follows the atom numbering: two numberings of one system can get different Kekule structures, and only
 *     mnx_normalize_pack behind this call makes them one form again, where its rule finds the rings (not in azulene);
 *   an aromatic ring drawn with a wedge (type 5 or 6 inside a ring of lower-case atoms) loses nothing here: the wedge is no type-4
 *     record and keeps its fields; mnx_normalize_pack behind this call loses it;
 *   a system that holds an upper-case atom on a type-4 bond is left untouched, and so is one with no matching (c1cccc1,
 *     triangulene) or one whose search runs beyond max_steps;
 *   the search is serial inside one system: one lane of the workgroup per system.
 *
 * Output. mols_out[b]: n_atoms and n_bonds of the input, smiles_len the length of the new text, which is the atoms' symbols behind
 * one another in atom order (NO token SMILES); flags = bit 0 copied | MNX_MOL_KEKULIZED (a system was rewritten) |
 * MNX_MOL_KEKULE_LEFT (a system stayed aromatic); the MNX_MOL_EXPAND* and mnx_normalize_pack's bits of the input are not copied. An
 * atom record keeps index, x_bin, y_bin and score; a bond record i, j and score; overall_score is copied.
 * MNX_MOL_KEKULIZE_REFUSED: as MNX_MOL_NORMALIZE_REFUSED — records beyond the tables passed, a symbol beyond n_text_bytes, a bond
 * whose i or j is no atom of the molecule, or more than 999 atoms or bonds; n_atoms = n_bonds = smiles_len = 0 in mols_out then.
 * atom_notes uint8 [atom_cap] (may be null): for output atom atom0 + k, bits 0-3 H of an aromatic atom (0 for every other atom),
 * MNX_NOTE_KEKULIZED: rewritten by this call, MNX_NOTE_KEKULE_LEFT: an aromatic atom that stayed as it came, with
 * MNX_NOTE_KEKULE_LIMIT when the step limit was the reason, MNX_NOTE_COPIED: no aromatic atom.
 * Inputs, outputs, the sizing protocol with totals [4] and the capped stores are mnx_normalize_pack's; max_steps stands in front of
 * stream. mnx_set_symbol_tables must have been called. Deterministic word for word: every position comes from a prefix scan, the
 * search of a system is serial, and the atomics of the kernel only count, add up, set bits of sets and take the minimum of a set.
 * Three launches, asynchronous on `stream`, no allocation, no host synchronisation.
 * MNX_ERR_INVALID_ARG (with mnx_last_error, "mnx_kekulize_pack: ..."): a null pointer (a table with capacity 0 may be null), n
 * outside 1..65536, misaligned records, or no symbol tables set; nothing is launched then. */
#define MNX_MOL_KEKULIZED 128u
#define MNX_MOL_KEKULE_LEFT 256u
#define MNX_MOL_KEKULIZE_REFUSED 512u
#define MNX_NOTE_KEKULIZED 16u
#define MNX_NOTE_KEKULE_LEFT 32u
#define MNX_NOTE_KEKULE_LIMIT 128u
#define MNX_KEKULE_DEFAULT_STEPS 16384u
int mnx_kekulize_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                      const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_mol* mols_out,
                      mnx_atom* atoms_out, uint32_t atom_cap, mnx_bond* bonds_out, uint32_t bond_cap, char* text_out,
                      uint32_t text_cap, uint8_t* atom_notes, uint32_t* totals, uint32_t max_steps, void* stream);

/* SMILES text read into the packed molecule tables, on the device: the inverse of mnx_smiles_pack. Strings in, mnx_mol / mnx_atom /
 * mnx_bond records and a text arena out, as mnx_graph_pack writes them, so that mnx_smiles_pack_canonical, mnx_expand_pack,
 * mnx_molfile_pack and the other writers run on a caller's own molecules unchanged: a gold column or a list of known compounds gets
 * the same canonical string as a prediction of the same graph. NO toolkit has parsed or produced any of these strings: this reader
 * and the writers are each other's check, no more. The grammar is the OpenSMILES one without its stereo and without '~' and '$'; a
 * bracket atom's bytes are COPIED, not interpreted (interpretation stays with the writers, which need mnx_set_symbol_tables; this
 * call needs no tables). No kekulisation, no hydrogen counting, no normalisation of [CH] against C here: aromatic rings, hydrogen
 * counts and brackets are mnx_normalize_pack's, behind this call.
 *
 * String b is bytes[offsets[b] .. offsets[b+1]). The rule, on the bytes of one string, positions counted from its first byte:
 * Brackets. A byte other than '[' and ']' is INSIDE when the nearest bracket in front of it is a '['. A '[' must be followed, as its
 *   next bracket, by a ']' that is not the very next byte; a ']' must have a '[' as the nearest bracket in front of it.
 * Tokens, from the bytes that are not inside:
 *   atom     one of B C N O P S F I b c n o p s * (Cl and Br: a C followed by l, a B followed by r, are one atom of two bytes), or a
 *            '[' with everything up to its ']' (one or more bytes, none of them a bracket). Atom k is the k-th atom token.
 *   bond     - = # : / \      branch  ( and )      dot  .
 *   ring     a digit 0..9, or '%' followed by two digits (numbers 00..99; '%' with anything else is an illegal byte; the two
 *            digits are part of the token). Numbers 0, 00 and 0 .. 9 against 00 .. 09 are the same numbers.
 *   illegal  every other byte, '~' and '$' among them, an l not behind C, an r not behind B, a stray ']'.
 * The current atom: none at the start and behind a '.'; behind an atom token that atom; behind a ')' the atom that was current in
 *   front of the matching '('. '(' leaves it as it is.
 * Bonds. An atom token bonds to the current atom, if there is one. A ring token whose number is not open opens it at the current
 *   atom; the next token with that number closes it: a bond between the atom that opened and the current atom, and the number is
 *   free again (first occurrence opens, second closes, whatever stands between them). A bond token belongs to the atom or ring
 *   token directly behind it. The type of a bond: '-' '/' '\' 1, '=' 2, '#' 3, ':' 4, from the bond token of a chain bond or of
 *   either end of a ring bond (both ends may carry the same symbol); with no symbol 4 when both atoms are spelled in lower case,
 *   else 1. An unbracketed atom is lower case by its first byte, a bracket atom by the first byte behind '[' and the digits that
 *   follow it ([nH], [13cH], [se]: lower case; [2*]: not).
 * Output of an admitted string: mols[b].n_atoms / n_bonds / smiles_len (the string's length; the molecule's text IS the string,
 *   copied), flags = 0, reserved = 0, overall_score = 0. Atom k: sym0 / sym_len its token's span in the text, brackets included,
 *   index = k, x_bin = y_bin = 0, score = 0. One bond record per bond: i < j in atom numbers, type, rev = type, score = 0; records
 *   sorted by i, then j (what mnx_graph_pack writes and mnx_expand_pack requires). recs[b]: flags, err_pos = 0, n_rings = bonds -
 *   atoms + components, where the components are the parts the '.' separate (1 + the number of '.'): the number of ring bonds. It
 *   exceeds the cycle rank of the graph where a ring number joins two parts across a '.' ("C1.C1": one ring bond, no cycle).
 *   MNX_READ_STEREO_DROPPED (not a refusal): the string holds a '/' or '\' bond token or an '@' inside a bracket atom. The bond is
 *   single; the '@' stays in the text and the writers drop it.
 *   The empty string is the empty molecule with flags 0.
 * Refusals. A refused string is the empty molecule: n_atoms = n_bonds = smiles_len = 0, mols[b].flags = 0, and recs[b].flags holds
 *   one bit only, tested in this order:
 *   MNX_READ_BEYOND     offsets[b] > offsets[b+1], or offsets[b+1] > n_bytes. No byte is read.
 *   MNX_READ_TOO_LARGE  more than 4096 bytes, or more than 999 atom tokens (the writers' limits); the string is examined no further.
 *   MNX_READ_SYNTAX     err_pos = the LOWEST position named by any of the following, each of which stands for itself whatever else
 *                       is wrong with the string (parentheses are matched as a stack that drops a ')' with nothing open; ring
 *                       numbers open and close by occurrence; the current atom is as stated above):
 *     an illegal byte: its position; a '[' whose next bracket is a '[' or that has none behind it, and "[]": the '[';
 *     a bond token whose next token is no atom and no ring token (or that is the last token): the bond token;
 *     a bond token that is the first token of the string or the first behind a '.';
 *     a ring token, '(', ')' or '.' that is the first token of the string, the first behind a '.' or behind a '(', or that is
 *       separated from one of these only by bond tokens: "()" , "((", "C(1", "C.1", "C(=1" break here;
 *       so a ring token behind a ')' is admitted and belongs to the atom in front of the '(' ;
 *     a '.' while a '(' is open; a '.' whose next token is no atom (or that is the last token): the '.';
 *     a ')' with no '(' open; a '(' that is never closed: the '(' (the lowest, if several);
 *     a ring number that is still open at the end: the token that opened it;
 *     a ring token that closes with a symbol that differs from the opening token's symbol ('/' against '\' too), onto the atom
 *       that opened it ("C11"), or onto a pair of atoms that has a bond already, be it a chain bond or an earlier ring bond
 *       ("C1C1", "C12CCC12"): the closing token (of the later bond).
 *   MNX_READ_TOO_LARGE  otherwise, more than 999 bonds.
 * Examples (atoms; bonds i-j:type): "CCO" 3; 0-1:1 1-2:1. "CC(=O)[O-]" 4; 0-1:1 1-2:2 1-3:1. "c1ccccc1" 6; 0-1:4 0-5:4 1-2:4 2-3:4
 *   3-4:4 4-5:4, n_rings 1. "c1ccccc1-c1ccccc1" 12; 5-6:1 among 13 bonds. "C1CC1.C1CC1" n_rings 2. "C%12CC%12" and "C0CC0" as
 *   "C1CC1". "C=1CC1" and "C1CC=1" 0-1:1 0-2:2 1-2:1. "F/C=C/F" 0-1:1 1-2:2 2-3:1, STEREO_DROPPED. "[13CH3][C@@H](N)C(=O)O" 6
 *   atoms, atom 0 = text[0..7), STEREO_DROPPED. "C(C)(C)(C)C" 0-1 0-2 0-3 0-4. "[Ph]C" 2 atoms (mnx_expand_pack expands the
 *   first). "Cl" 1 atom of 2 bytes; "ClC" 2 atoms.
 *
 * Inputs, device pointers: bytes [n_bytes] (may be null when n_bytes is 0), offsets uint32 [n + 1], 1 <= n <= 65536.
 * Outputs, device pointers the caller allocated: mols [n], recs [n]; atoms [atom_cap], bonds [bond_cap] (8-byte aligned), text
 * [text_cap]; totals uint32 [4] = {atoms, bonds, text bytes needed, 1 if any capacity was too small}. When a capacity is too small
 * nothing is written beyond it, and mols, recs and totals are complete all the same: read the needed sizes and call again. A table
 * of capacity 0 may be null. Deterministic word for word (every position comes from a prefix scan or a rank; no atomic decides a
 * position or an order); records are written whole, padding bytes as zeros. Three launches, asynchronous on `stream`, no allocation,
 * no host synchronisation.
 * MNX_ERR_INVALID_ARG (with mnx_last_error, "mnx_smiles_read: ..."): a null pointer, n outside 1..65536, misaligned records (mols,
 * atoms, bonds 8-byte; recs, offsets, totals 4-byte); nothing is launched then. */
typedef struct mnx_read {
    uint32_t flags;             /* MNX_READ_* */
    uint32_t err_pos;           /* MNX_READ_SYNTAX: the lowest position at which a rule breaks; else 0 */
    uint32_t n_rings;
    uint32_t reserved;          /* 0 */
} mnx_read;
#define MNX_READ_SYNTAX 1u
#define MNX_READ_TOO_LARGE 2u
#define MNX_READ_STEREO_DROPPED 4u
#define MNX_READ_BEYOND 8u
int mnx_smiles_read(mnx_engine* h, const char* bytes, uint32_t n_bytes, const uint32_t* offsets, int32_t n, mnx_mol* mols,
                    mnx_read* recs, mnx_atom* atoms, uint32_t atom_cap, mnx_bond* bonds, uint32_t bond_cap, char* text,
                    uint32_t text_cap, uint32_t* totals, void* stream);

/* V2000 molfiles read on the device into the packed tables: the inverse of mnx_molfile_pack. A molfile carries what the stereo
 * writers read and a SMILES cannot — 2D coordinates and wedge flags —, so through this call the stereo of a caller's own molecule
 * reaches mnx_smiles_pack_stereo / _marks / _canonical / _symmetric, the fingerprints and every pass; and the molfile writer has a
 * reader that is its check. File b is bytes[offsets[b] .. offsets[b+1]). Everything not said here is as in mnx_smiles_read: the
 * outputs, totals[4], the capacity protocol, three launches, asynchronous, no allocation, no host synchronisation, deterministic
 * word for word, records written whole. No symbol tables are needed. den = cfg.coord_bins - 1, as in mnx_molfile_pack.
 * THE RULE IS THIS LIBRARY'S OWN: the format is the CTfile specification's, the spelling of an atom (brackets, hydrogens, lower
 * case, '@') is what makes mnx_molfile_pack's own files come back as the tables they were written from. It is NOT a toolkit's
 * valence or aromaticity model, and no toolkit has read these tables.
 *
 * scale: device int32 [n, 2] = {Sx, Sy} in units of 1e-4, each clamped to 1..10000000; null: 100000 each — the writer's argument
 *   with the writer's meaning. fit: 0 or 1; fit = 1 with a scale is an argument error.
 * Lines end with '\n'; one '\r' directly in front of it is dropped; the last line may lack the '\n'. A byte a line does not have
 *   reads as a blank. A numeric field "%3d" is its bytes with blanks trimmed: empty = 0, else an optional '-' and 1 to 3 digits;
 *   anything else breaks the rule at that line.
 * Layout. Lines 1 to 3 are ignored. Line 4 holds the atom count in columns 1-3 and the bond count in 4-6 (negative: SYNTAX);
 *   "V3000" anywhere on it is SYNTAX at line 4. Then the atom lines, the bond lines and the property block. Nothing behind the
 *   FIRST line that begins "M  END" — whatever that line would otherwise be — is ever read: SDF data items and "$$$$" may follow.
 *   A file without such a line is SYNTAX at (number of lines + 1); so is a line the layout needs and the file, cut behind its
 *   "M  END" line, does not have: at (lines read + 1). A file of zero bytes is the empty molecule with flags 0.
 * Atom line k (line 4 + k): shorter than 31 bytes is SYNTAX. Columns 1-10 x, 11-20 y (z is not read): blanks, an optional '-',
 *   one or more digits, optionally '.' and zero or more digits, nothing else; the value in units of 1e-4 is the integer part *
 *   10000 + the first four fraction digits right-padded with zeros. Columns 32-34 the symbol, blanks trimmed; 35-36 the mass
 *   difference (nonzero: IGNORED); 37-39 the charge code 0 -> 0, 1 -> +3, 2 -> +2, 3 -> +1, 4 -> 0 with IGNORED, 5 -> -1, 6 -> -2,
 *   7 -> -3, else SYNTAX; 49-51 the valence v, 0..15, else SYNTAX.
 * Bond line: a1, a2, type, stereo in columns 1-3, 4-6, 7-9, 10-12. a1 and a2 in 1..atoms and different, else SYNTAX. Type 1..4;
 *   5..8 refuses the file with QUERY; else SYNTAX. Stereo 0 none; 1 class 5 and 6 class 6, on type 1 only; 4 on type 1 and 3 on
 *   type 2 a plain bond with STEREO_EITHER; anything else SYNTAX. A wedge line "begins at" a1. The record has i < j: a1 < a2
 *   gives (a1, a2, cls, flip(cls)), a1 > a2 gives (a2, a1, flip(cls), cls), flip: 5 <-> 6. Records sorted by i, then j. The same
 *   pair on two lines is SYNTAX at the later line.
 * Property block, up to "M  END". "A  nnn": the next line is the alias of atom nnn (an empty one: no alias; more than 70 bytes:
 *   SYNTAX at it; no line in front of "M  END": SYNTAX at the "A  " line); bytes below 0x20 and 0x7f are stored as '?'. A line
 *   that is an alias's text is nothing else, whatever it begins with. "M  CHG", "M  ISO", "M  RGP": a count of 1..8 in columns
 *   7-9 and entries " aaa vvv" from column 10 + 8e; CHG values -15..15, ISO and RGP 0..999; an atom or value out of range is
 *   SYNTAX. The first "M  CHG" line resets every atom-block charge to 0. Of two entries of one kind (or two aliases) for one atom
 *   the later in file order wins. Every other line is skipped and sets IGNORED.
 * One atom's symbol; the molecule's text is the symbols behind one another, smiles_len their total length (no SMILES). s: the sum
 *   of its bond orders (classes 1, 5, 6 count 1, 2 counts 2, 3 counts 3, 4 counts 0); arom: it has a class-4 bond.
 *   1 an alias: '[' alias ']', LABEL. 2 else "R#" with an RGP value n > 0: "[Rn]", LABEL. 3 "D" / "T": H with isotope 2 / 3, which
 *   an M ISO entry overrides. 4 "R", "R#", "A", "Q", "L", "X", "*" and the empty symbol: the element '*'. 5 any other symbol that
 *   is none of the 118 elements: '[' symbol ']', LABEL. 6 an element: lower case exactly when arom and it is one of B C N O P S
 *   Se As. Bracketed when it has a charge, an isotope or v != 0, is outside B C N O P S F Cl Br I '*', or is marked. H of a
 *   bracket atom: v != 0 and not arom: max(0, (v == 15 ? 0 : v) - s); arom: 0 (the writer's own known limit: [nH] comes back as
 *   n); else from the table B 3, C 4, N 3|5, O 2, P 3|5, S 2|4|6, F Cl Br I 1, N+ P+ 4, O+ S+ C+ C- 3, N- 2, O- S- 1, B- 4 — the
 *   smallest target >= s, minus s, 0 without one — with H_DEFAULT set; above 9 written as 9. Marked: an upper-case C with charge
 *   0 and isotope 0 at which a wedge line begins and whose H (computed as above, bracketed or not) is <= 1. Spelled '[' isotope?
 *   element '@'? ('H' | 'Hn')? ('+' | '-' | sign and 2..15)? ']', or the bare element. Only '@' is ever written: the writers read
 *   a mark's presence, not its sense.
 * Records: index = k, every score 0, mols[b].flags = 0. Bins with fit = 0: xb = (2 ux den + Sx) / (2 Sx), yb = den - (2 uy den +
 *   Sy) / (2 Sy) in integers; a negative coordinate gives 0 before the subtraction, a result above den gives den, either sets
 *   CLAMPED. This is the exact inverse of the writer whenever S > den: the writer's rounding moves u by at most 1/2, that is the
 *   quotient by at most den / (2 S) < 1/2. fit = 1: with minx, miny and span = max(maxx - minx, maxy - miny, 1) over the file's
 *   atoms, xb = (2 (ux - minx) den + span) / (2 span), yb = den - the same in y: one uniform scale, never CLAMPED.
 * Refusals. A refused file is the empty molecule with exactly one of the bits, tested in this order: BEYOND (the offsets are out
 *   of order or lie beyond n_bytes); TOO_LARGE (more than 262144 bytes, or more than 8192 lines with no "M  END" among the first
 *   8192; three columns hold no count above 999); SYNTAX or QUERY with err_line = the lowest 1-based line at which a rule
 *   breaks — SYNTAX where both break at that line.
 * Limits. Reading is the inverse of mnx_molfile_pack on what a drawing holds — wedges from [C@H] / [C@] to a neighbour that is
 *   no such centre, rev = flip(type), lower-case atoms on class-4 bonds —, not a projection on arbitrary tables: a plain C at
 *   which a wedge begins comes back as [C@H], a wedge between two centres changes its owner, [nH] comes back as n. An alias's
 *   text that begins "M  END" ends the file.
 * Examples: "\n\n\n  2  1\n<C at 1.0 2.0>\n<O at 0 0>\n  1  2  1  0\nM  END\n" -> 2 atoms "C" "O", text "CO", bond (0, 1, 1, 1).
 *   The same bond line as "  2  1  1  1": (0, 1, 6, 5). An atom "N" with "M  CHG  1   1   1" and v = 4, no bonds: "[NH4+]".
 *
 * MNX_ERR_INVALID_ARG (with mnx_last_error, "mnx_molfile_read: ..."): a null pointer, n outside 1..65536, fit outside 0..1 or
 * fit = 1 with a scale, cfg.coord_bins below 2, misaligned records (mols, atoms, bonds 8-byte; recs, offsets, scale, totals
 * 4-byte); nothing is launched then. */
typedef struct mnx_molread {        /* 16 bytes, like mnx_read */
    uint32_t flags;                 /* MNX_MOLREAD_* */
    uint32_t err_line;              /* refusal by SYNTAX / QUERY: the lowest 1-based line at which a rule breaks; else 0 */
    uint32_t n_marked;              /* atoms spelled with '@' */
    uint32_t reserved;              /* 0 */
} mnx_molread;
#define MNX_MOLREAD_SYNTAX 1u          /* refusals: exactly one of bits 0, 1, 3, 4 */
#define MNX_MOLREAD_TOO_LARGE 2u
#define MNX_MOLREAD_BEYOND 8u
#define MNX_MOLREAD_QUERY 16u
#define MNX_MOLREAD_STEREO_EITHER 32u  /* notes, not refusals */
#define MNX_MOLREAD_H_DEFAULT 64u
#define MNX_MOLREAD_CLAMPED 128u
#define MNX_MOLREAD_IGNORED 256u
#define MNX_MOLREAD_LABEL 512u
int mnx_molfile_read(mnx_engine* h, const char* bytes, uint32_t n_bytes, const uint32_t* offsets, int32_t n,
                     const int32_t* scale, int32_t fit, mnx_mol* mols, mnx_molread* recs, mnx_atom* atoms, uint32_t atom_cap,
                     mnx_bond* bonds, uint32_t bond_cap, char* text, uint32_t text_cap, uint32_t* totals, void* stream);

/* Path fingerprints, on the device: of every packed molecule a set of 2048 bits that says which paths of atoms and bonds it holds,
 * and (mnx_tanimoto, below) the similarity of two such sets. Everything else at the end of the chain of passes is a yes or a no —
 * the same canonical string or not —; this is the graded answer: how far a prediction is from its gold structure, which known
 * compound is nearest. A sink like the writers, not a pass: packed tables in, a fixed-size record and 64 words per molecule out.
 * Intended order: mnx_graph_pack or mnx_smiles_read -> the passes -> mnx_kekulize_pack -> mnx_normalize_pack -> THIS CALL: behind
 * the last two an aromatic and a Kekule spelling of one ring give the same atoms and bonds and so the same bits.
 * THE RULE IS THIS LIBRARY'S OWN, after the idea of Daylight's and RDKit's path fingerprints. It does NOT produce RDKit's bits
 * (RDKFingerprint) and its similarities are not RDKit's: no toolkit is at hand to compare with, and none has seen these bits. The
 * reference's evaluate.py only names the metric and the path length of 7.
 *
 * Admission, as mnx_smiles_pack_canonical admits a molecule for its ranks, with the same bits and values: MNX_FP_TOO_LARGE (bit
 *   0) more than 999 atoms or 999 bonds; MNX_FP_BEYOND_TABLES (bit 1) its records, or a symbol, reach beyond the tables passed;
 *   MNX_FP_BAD_BOND (bit 4) the same atom pair in two bond records, a record with i == j, or an end that is no atom of the
 *   molecule. MNX_FP_PSEUDO_ATOM (bit 2) and MNX_FP_TRUNCATED (bit 3, a copy of MNX_MOL_TRUNCATED) are informational, as in
 *   mnx_smiles; a molecule refused on bit 0 or 1 has had no atom read and so never bit 2.
 * Atom key. k(a) = fmix32(fnv1a_bytes(text(a))), text(a) being the bytes a writer puts down for the atom without a stereo mark:
 *   the at most 12 bytes that the canonical ranks take as their initial key (mnx_smiles_pack_canonical), so 'C', 'c', '[NH3+]',
 *   '[13CH3]' differ, a pseudo-atom is '*' and a numbered R-group '[n*]'.
 * Bond word. 1 for a bond record of type 1, 5 or 6 (a wedge is a single bond), 2 for type 2, 3 for type 3, 4 for type 4, 5 for
 *   any other type. `rev` is not read.
 * Paths. A path is a sequence of distinct atoms a0 .. aL, consecutive ones joined by a bond record, 0 <= L <= max_bonds; L = 0 is
 *   the single atom. max_bonds is 1 .. MNX_FP_MAX_BONDS (7, the reference's maxPath); 0 means 7. A walk never returns to an atom
 *   it holds, so a ring is never closed: a ring of 6 is seen as its paths of up to 5 bonds.
 * Path hash. The word sequence of a path is k(a0), c1, k(a1), .., cL, k(aL). H(seq) is FNV-1a over 32-bit words: h = 2166136261,
 *   then h = (h ^ w) * 16777619 mod 2^32 for every word; fnv1a_bytes is the same over bytes. fmix32 is murmur3's finaliser: h ^= h
 *   >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16. The path's hash is p = fmix32(min(H(seq), H(seq
 *   reversed))): both ends of a path give one value, and so does every numbering of the atoms.
 * Bits. A path sets bit p & 2047 and bit (p >> 11) & 2047. Bit t is word t >> 5, mask 1u << (t & 31).
 * Step limit. For a directed bond s = (a -> n), P(s) is the number of paths of 1 .. max_bonds bonds that begin with it: a property
 *   of the graph, not of how the work is split. A molecule with any P(s) > max_steps gets MNX_FP_LIMIT (bit 16) and no bits.
 *   max_steps == 0 means MNX_FP_DEFAULT_STEPS; more than MNX_FP_MAX_STEPS is an argument error (a dense graph could otherwise
 *   hold a workgroup for minutes). The largest P(s) is 73 for taxol, 59 for coronene, 52 for atorvastatin — a drawn molecule is
 *   far from the limit —, 1957 for the complete graph on 8 atoms and 8660 for the one on 9.
 * A molecule refused on bit 0, 1 or 4, or limited, has all 64 words zero and n_bits 0. The empty molecule is admitted: no bits.
 * recs[b]: flags; n_bits, the number of bits set; max_paths, the largest P(s) — 0 without bonds or when refused, 0xFFFFFFFF when
 *   limited —; reserved 0.
 * Inputs as mnx_smiles_pack's: mols [n], 1 <= n <= 65536; atoms [n_atom_records], bonds [n_bond_records] (8-byte aligned), text
 * [n_text_bytes]; mnx_set_symbol_tables must have been called. Outputs, device pointers the caller allocated: recs [n], bits
 * uint32 [n][64] (4-byte aligned). Deterministic word for word: the bits are ORs and max_paths is a maximum in on-chip memory,
 * neither of which depends on the order of its operands; no atomic decides a position. Records and words are written whole. One
 * launch, asynchronous on `stream`, no allocation, no host synchronisation.
 * MNX_ERR_INVALID_ARG (with mnx_last_error, "mnx_fingerprint_pack: ..."): a null pointer (an input table of 0 records may be
 * null), n outside 1..65536, misaligned records, no symbol tables set, max_bonds above 7, max_steps above MNX_FP_MAX_STEPS;
 * nothing is launched then. */
typedef struct mnx_fp {
    uint32_t flags;             /* MNX_FP_* */
    uint32_t n_bits;            /* bits set in the molecule's 64 words */
    uint32_t max_paths;         /* the largest number of paths from one directed bond; 0xFFFFFFFF with MNX_FP_LIMIT */
    uint32_t reserved;          /* 0 */
} mnx_fp;
#define MNX_FP_TOO_LARGE 1u
#define MNX_FP_BEYOND_TABLES 2u
#define MNX_FP_PSEUDO_ATOM 4u
#define MNX_FP_TRUNCATED 8u
#define MNX_FP_BAD_BOND 16u
#define MNX_FP_LIMIT 65536u
#define MNX_FP_WORDS 64u
#define MNX_FP_MAX_BONDS 7u
#define MNX_FP_DEFAULT_STEPS 4096u
#define MNX_FP_MAX_STEPS (1u << 20)
int mnx_fingerprint_pack(mnx_engine* h, const mnx_mol* mols, int32_t n, const mnx_atom* atoms, uint32_t n_atom_records,
                         const mnx_bond* bonds, uint32_t n_bond_records, const char* text, uint32_t n_text_bytes, mnx_fp* recs,
                         uint32_t* bits, uint32_t max_bonds, uint32_t max_steps, void* stream);

/* The Tanimoto similarity of rows of fingerprints, pair by pair: row i of a against row i of b, each 64 words as
 * mnx_fingerprint_pack writes them. both[i] = popcount(a[i] & b[i]), either[i] = popcount(a[i] | b[i]), similarity[i] = (double)
 * both[i] / (double)either[i], and 0.0 when either[i] == 0: this library's own choice — an empty side is a refused, limited or
 * empty molecule, and that is a mismatch here as it is everywhere else. One correctly rounded division of two integers below
 * 2049: the same double on host and device. No all-pairs matrix: pass the rows paired as they are to be compared.
 * a, b: device uint32 [n][64], 1 <= n <= 65536 (they may be the same pointer). both, either: device uint32 [n]; similarity: device
 * double [n]; each of the three may be null, not all of them. One launch, asynchronous on `stream`, no allocation, no host
 * synchronisation; needs no tables.
 * MNX_ERR_INVALID_ARG (with mnx_last_error, "mnx_tanimoto: ..."): a or b null, all three outputs null, n outside 1..65536, a
 * pointer that is not 4-byte (similarity: 8-byte) aligned; nothing is launched then. */
int mnx_tanimoto(mnx_engine* h, const uint32_t* a, const uint32_t* b, int32_t n, uint32_t* both, uint32_t* either,
                 double* similarity, void* stream);

/* Nearest rows, on the device: for every row of `queries` the k rows of `library` that are nearest to it by the Tanimoto
 * similarity above — which known compound is nearest —, without the nq * nl pairs of rows ever being written down. Both are tables
 * of 64-word rows as mnx_fingerprint_pack writes them, and they may be the same pointer. THE FINGERPRINT IS THIS LIBRARY'S OWN, so
 * the neighbours are not those RDKit's fingerprints would give. There is no count of all rows above a threshold and k is at most
 * MNX_NEAREST_MAX_K (64).
 *
 * Pair quantities, for query q and library row r: both = popcount(Q & R), either = popcount(Q | R), s = (double)both /
 *   (double)either, and 0.0 when either == 0: exactly mnx_tanimoto's numbers for that pair.
 * Order. Row x comes before row y for a query if and only if both_x * either_y > both_y * either_x (a pair with either == 0
 *   counting as 0 / 1), or the two products are equal and index_x < index_y. A total order: the result cannot depend on how the
 *   work is split, on the grid, or on which wave arrives first. It is the order of the doubles s: two different fractions with
 *   denominators below 2049 differ by at least 1 / (2048 * 2047), far above one ulp, so each rounds to its own double.
 * Result per query: the first k rows in that order, 1 <= k <= MNX_NEAREST_MAX_K, of those the ones with s >= min_similarity (the
 *   cut of the sorted k equals a filter in front, so the double is computed k times per query). count[q] says how many were kept;
 *   index[q][j], both[q][j], either[q][j] and similarity[q][j] hold them for j < count[q], and MNX_NEAREST_NONE, 0, 0 and 0.0
 *   behind that. A library of fewer than k rows gives fewer.
 * flags. MNX_NEAREST_SKIP_SELF: library row q is no candidate for query q — the nearest OTHER row when a set is searched in
 *   itself. Any other bit is an argument error.
 * queries: device uint32 [nq][64], 1 <= nq <= MNX_NEAREST_MAX_QUERIES (4096); library: device uint32 [nl][64], 1 <= nl <=
 * MNX_NEAREST_MAX_ROWS (2^24); 0 <= min_similarity <= 1. Outputs, device pointers the caller allocated: count uint32 [nq]; index,
 * both, either uint32 [nq][k]; similarity double [nq][k]; written whole. both, either and similarity may each be null, count and
 * index may not. work: device scratch of at least mnx_tanimoto_search_work_bytes(nq, nl, k) bytes, 8-byte aligned; what it holds
 * after the call is unspecified. That size is 8 * k * min(nq * min(MNX_NEAREST_MAX_LISTS, slabs), 32768 + nq) bytes with slabs =
 * ceil(nl / MNX_NEAREST_SLAB_ROWS): never more than nq * k * 8 * MNX_NEAREST_MAX_LISTS, monotone in each argument, and 0 for
 * arguments the call would refuse.
 * Geometry (exported because tests take their shapes from it): a workgroup holds MNX_NEAREST_QUERY_TILE queries at once and walks
 * slabs of MNX_NEAREST_SLAB_ROWS library rows; a query has at most MNX_NEAREST_MAX_LISTS partial lists of k candidates in `work`,
 * merged by the second launch. Deterministic word for word: no atomic, global or on chip. Two launches, asynchronous on `stream`,
 * no allocation, no host synchronisation; needs no tables.
 * MNX_ERR_INVALID_ARG (with mnx_last_error, "mnx_tanimoto_search: ..."): queries, library, count, index or work null; nq outside
 * 1..4096, nl outside 1..2^24, k outside 1..64; min_similarity NaN or outside [0, 1]; an unknown flag bit; work_bytes too small; a
 * word pointer that is not 4-byte aligned, similarity or work not 8-byte; nothing is launched then. */
#define MNX_NEAREST_MAX_K 64u
#define MNX_NEAREST_MAX_QUERIES 4096u
#define MNX_NEAREST_MAX_ROWS (1u << 24)
#define MNX_NEAREST_NONE 0xFFFFFFFFu
#define MNX_NEAREST_SKIP_SELF 1u
#define MNX_NEAREST_QUERY_TILE 32u
#define MNX_NEAREST_SLAB_ROWS 256u
#define MNX_NEAREST_MAX_LISTS 512u
size_t mnx_tanimoto_search_work_bytes(int32_t nq, uint32_t nl, uint32_t k);
int mnx_tanimoto_search(mnx_engine* h, const uint32_t* queries, int32_t nq, const uint32_t* library, uint32_t nl, uint32_t k,
                        double min_similarity, uint32_t flags, uint32_t* count, uint32_t* index, uint32_t* both,
                        uint32_t* either, double* similarity, void* work, size_t work_bytes, void* stream);

/* Substructure search, on the device: for pairs of a QUERY molecule Q and a TARGET molecule T, each one molecule of a set of packed
 * tables (the two sets may be the same), whether Q embeds in T, how often, and where: the first embedding as a map from Q's atoms
 * to T's, whose mnx_atom records carry the coordinate bins — a scaffold found is a place on the page. Run in both directions on
 * molecules with equal atom and bond counts it is a test of graph isomorphism that depends on no canonical ranking (the ranks have
 * a KNOWN LIMIT, mnx_smiles_pack_canonical). A sink like mnx_fingerprint_pack: packed tables in, a record and a map per pair out.
 * Intended order: both sides -> the passes -> mnx_kekulize_pack -> mnx_normalize_pack -> THIS CALL, so that both have one spelling.
 * THE RULE IS THIS LIBRARY'S OWN. It is NOT RDKit's HasSubstructMatch, it is not SMARTS, and no toolkit has checked it.
 *
 * Admission. Each side is admitted exactly as mnx_fingerprint_pack admits a molecule. The target's bits stand in flags bits 0-4
 *   with the MNX_FP_* values, the query's in bits 8-12 (the same values << MNX_MATCH_QUERY_SHIFT); bits 2 and 3 (10 and 11) are
 *   informational. MNX_MATCH_QUERY_TOO_LARGE (bit 5): a query that is otherwise admitted has more than MNX_MATCH_MAX_QUERY (64)
 *   atoms or more than MNX_MATCH_MAX_QUERY_BONDS (128) bonds. MNX_MATCH_QUERY_EMPTY (bit 6): an admitted query has no atom.
 *   MNX_MATCH_BAD_PAIR (bit 17): the pair names a molecule index outside either table — the indices are device data, so this is
 *   no argument error; no other bit is set then. The refusing bits are 0, 1, 4, 8, 9, 12, 5, 6 and 17: a refused pair has
 *   n_matches 0, steps 0 and a map of all 0xFFFF. Both sides' bits are always reported, whichever refuses.
 * Atom match, query atom q against target atom t. q is a WILDCARD when it is a pseudo-atom, a numbered R-group, or an atom whose
 *   element a writer puts down as '*'; a wildcard matches every target atom. Otherwise t must be a plain atom, not itself spelled
 *   '*', with the same element, the same aromatic (lower-case) bit and the same charge, and the same isotope unless q's isotope is
 *   0. LIMITS: H counts and brackets are NOT compared ('[NH4+]' matches '[N+]', 'N' matches '[NH2]'), and stereo is NOT compared
 *   (wedges count as single bonds, '@' marks were dropped by the readers). deg(q) <= deg(t) follows; it is no separate condition.
 * Bond match. A bond record's class is 0 for type 1, 5 or 6 (a wedge is a single bond), 1 for type 2, 2 for type 3, 3 for type 4
 *   and 4 (ANY) for every other type. A query bond of class ANY matches every target bond; any other class matches a target bond
 *   of the same class only (a target bond of class ANY is matched by a query bond of class ANY alone). `rev` is not read.
 * Embedding. An injective map of Q's atoms into T's atoms such that every pair of atoms matches and every query bond lies on a
 *   matching target bond. Further target bonds among the images are allowed — the match is NOT induced: propane embeds in
 *   cyclopropane, cyclopropane does not embed in propane. Embeddings are counted as maps: benzene embeds 12 times in toluene.
 * Order of the query atoms. Breadth first from the lowest-numbered atom not yet placed, an atom's neighbours in ascending index,
 *   repeated until every atom is placed (a disconnected query is supported). Position k has parent[k], its breadth-first parent;
 *   the first atom of each component has none. This order defines "the first embedding" and the steps.
 * Candidates. At position 0 each target atom in turn is the ROOT of a search of its own. At a later position with a parent the
 *   candidates are the neighbours of the parent's image in ascending target index; at the first atom of a later component they
 *   are all target atoms, ascending. A candidate is ACCEPTED when it is not yet an image, the atoms match, and every query bond
 *   from this atom to an atom placed earlier has a matching target bond.
 * Steps. Every candidate examined costs one step, whatever rejects it, and so does the root. The depth-first search from root r
 *   ends when it runs out of candidates, when it reaches its max_matches-th embedding, or when its step count S(r) passes
 *   max_steps (it is then BROKEN OFF).
 * Results. n_matches = min(max_matches, the sum over all roots of the embeddings found). steps = the maximum over the roots of
 *   S(r), max_steps + 1 for a search broken off. MNX_MATCH_LIMIT (bit 16): some root was broken off and n_matches < max_matches
 *   — the count is then a lower bound; n_matches >= 1 is a certain yes with or without bit 16. The map: the first embedding of
 *   the lowest root that has one — the lexicographically smallest image sequence along the order —, maps[p][a] the image of query
 *   atom a, 0xFFFF beyond the query's atoms or without a match. All of these are properties of the two graphs, not of how the
 *   roots are dealt to lanes: no search stops because another has found something.
 * max_matches: 0 means 1; more than 65535 is an argument error. max_steps: 0 means MNX_MATCH_DEFAULT_STEPS; more than
 *   MNX_MATCH_MAX_STEPS is an argument error (a dense graph must not park a workgroup for minutes).
 *   Measured with the oracle of tests/substructure_ref.py, the largest S(r) at max_matches 1 / 65535: benzene in coronene 18 / 131,
 *   naphthalene in coronene 105 / 175, an aromatic 12-ring in coronene 160 / 1397, an aromatic 12-chain in coronene 22 / 709, the
 *   cholest-5-ene core in cholesterol 89 / 110 (the saturated gonane core, which the double bond keeps out: 131 / 131), the taxane
 *   core in taxol 59 / 85, coronene in itself 423 / 423, an aromatic 18-ring in coronene 100 / 3739, aromatic chains of 24 and 25
 *   atoms in coronene (24 atoms) 3063 / 3805 and 3815 / 3815; the 64 random pairs of tests/test_gpu_substructure.py 23 / 25. The
 *   default is the next power of two at least 16 times above the largest, 3815. LIMIT: no all-carbon query in these polycycles came
 *   near 1 << 20, but a dense target does — a chain of seven C and one N in the complete graph on nine C takes 231689 steps to be
 *   refuted and is reported with bit 16 at the default, not searched to the end.
 * recs[p]: flags; n_matches; steps; reserved 0.
 * Inputs: the two sides as mnx_fingerprint_pack's input side, 1 <= nq, nt <= 65536; pairs: device uint32 [n_pairs][2], the query
 * index then the target index, 1 <= n_pairs <= 1048576; mnx_set_symbol_tables must have been called. Outputs, device pointers the
 * caller allocated: recs [n_pairs], maps uint16 [n_pairs][MNX_MATCH_MAX_QUERY]. Deterministic word for word: the embeddings are
 * summed, the steps a maximum and the winning root a minimum in on-chip memory, none of which depends on the order of its
 * operands; no atomic decides a result. Records and maps are written whole. One launch, asynchronous on `stream`, no allocation,
 * no host synchronisation.
 * MNX_ERR_INVALID_ARG (with mnx_last_error, "mnx_substructure_match: ..."): a null pointer (an input table of 0 records may be
 * null), nq or nt outside 1..65536, n_pairs outside 1..1048576, misaligned pointers (records 8-byte, pairs and recs 4-byte, maps
 * 2-byte), no symbol tables set, max_matches above 65535, max_steps above MNX_MATCH_MAX_STEPS; nothing is launched then. */
typedef struct mnx_match {
    uint32_t flags;             /* MNX_FP_* of the target, the same << MNX_MATCH_QUERY_SHIFT of the query, MNX_MATCH_* */
    uint32_t n_matches;         /* embeddings found, max_matches at the most */
    uint32_t steps;             /* the longest search of one root; max_steps + 1 when one was broken off */
    uint32_t reserved;          /* 0 */
} mnx_match;
#define MNX_MATCH_QUERY_TOO_LARGE 32u
#define MNX_MATCH_QUERY_EMPTY 64u
#define MNX_MATCH_QUERY_SHIFT 8
#define MNX_MATCH_LIMIT 65536u
#define MNX_MATCH_BAD_PAIR 131072u
#define MNX_MATCH_MAX_QUERY 64u
#define MNX_MATCH_MAX_QUERY_BONDS 128u
#define MNX_MATCH_DEFAULT_STEPS 65536u
#define MNX_MATCH_MAX_STEPS (1u << 20)
int mnx_substructure_match(mnx_engine* h,
                           const mnx_mol* q_mols, int32_t nq, const mnx_atom* q_atoms, uint32_t q_atom_records, const mnx_bond* q_bonds,
                           uint32_t q_bond_records, const char* q_text, uint32_t q_text_bytes,
                           const mnx_mol* t_mols, int32_t nt, const mnx_atom* t_atoms, uint32_t t_atom_records, const mnx_bond* t_bonds,
                           uint32_t t_bond_records, const char* t_text, uint32_t t_text_bytes,
                           const uint32_t* pairs, int32_t n_pairs, mnx_match* recs, uint16_t* maps,
                           uint32_t max_matches, uint32_t max_steps, void* stream);

/* mnx_predict with beam search (BASELINE config 5): the same inputs and outputs, every reference batch searched as
 * mnx_decode_beam does (n_best = 1: the best hypothesis; atom positions and the bond head run on ITS tokens and decoder
 * outputs) while the encoder of the following launch groups runs on the second stream. Up to MNX_BEAM_GROUPS (environment,
 * default 8; bounded by 256 images and by dec_slots rows) reference batches of an encoder launch group share ONE step
 * sequence — 8 x 32 x 5 = 1280 rows per step —: images are independent but for the positional-encoding row, which is numbered
 * inside each image's own reference batch, so the hypotheses are exactly those of batch-by-batch searches (2.3x the
 * throughput of one batch at a time). Replaces `decoder.decode(features, hiddens, beam_size=beam)` inside the chunk loop of
 * predict_images (MolNexTR/model.py:102-109, components.py:443) — a branch the reference itself cannot execute (see
 * mnx_decode_beam).
 *   scores    device fp32 [n_img]: average log-prob of the returned hypothesis
 * Synchronous with respect to its outputs. */
int mnx_predict_beam(mnx_engine* h, const float* images, int32_t n_img, int32_t ref_batch, int32_t beam, int32_t max_len,
                     int32_t* tokens, int32_t* lengths, float* scores, int32_t* n_atoms, int32_t* atom_idx,
                     uint8_t* edges, int32_t kmax, void* stream);

/* Kernel-level timing aid for bench.py: runs the 16-bit MFMA GEMM of the encoder on caller buffers.
 * C[M,N] = A[M,K] . W[N,K]^T + bias, A/W 16-bit device, epi: 0 bias->16-bit, 1 bias+GELU->16-bit,
 * 2 bias+residual(fp32, in place in C), 3 bias->fp32. epi | 0x100 (epi 2, 3; test aid) runs the persistent fp32-output
 * kernel (gemm_res.hip) whatever the shape dispatch would choose.
 * Refused before any launch with MNX_ERR_INVALID_ARG and an error text that starts with the function's name (both entry
 * points): a null A, W or C, M <= 0, K or N not a positive multiple of 8 (FP32 engines: K of 16), and | 0x100 on a shape or
 * epilogue gemm_res.hip does not support (M % 256, N % 128, K % 64, N <= 1024; plain operands: K >= 128). */
int mnx_gemm16(mnx_engine* h, int32_t epi, const void* A, const void* W, void* C, const float* bias, int32_t M,
               int32_t N, int32_t K, void* stream);

/* The same for the split modes (the engine's compute_dtype must be BF16X3 / FP16X3): A, W (and C for epi 0 / 1) point at
 * hi planes, a_lo / w_lo / c_lo are the ELEMENT offsets of the lo planes, C = epi(oscale * (Ah.Wh + Ah.Wl + Al.Wh) + bias)
 * with the exact-erf GELU; terms = 3, 2 (Ah.Wh + Ah.Wl: a_lo is ignored; FP16X3 / FP16X3M engines) or 1 (Ah.Wh alone).
 * Test aids in `epi`: | 0x100 the persistent fp32-output kernel of gemm_res.hip, | 0x200 the 128x128 kernel whatever the
 * dispatch would choose, | 0x400 (epi 0 / 1) write the hi output plane only (c_lo ignored). */
int mnx_gemm16_split(mnx_engine* h, int32_t epi, const void* A, int64_t a_lo, const void* W, int64_t w_lo, float oscale,
                     void* C, int64_t c_lo, const float* bias, int32_t M, int32_t N, int32_t K, int32_t terms,
                     void* stream);

/* Test aid: the encoder's window attention (12x12 windows, head_dim 32) on caller device buffers, with the engine's
 * compute_dtype. qkv [B*H*W, 3C] and out [B*H*W, C] are token-major in the original (unshifted) token order, table is the
 * reference's relative_position_bias_table, fp32 [(2*12-1)^2, heads] (the layout mnx_create uploads). shift = 0 or
 * 1..11 (the cyclic shift and its -100 region mask, as the encoder's odd blocks run it with 6). Split compute_dtypes
 * (BF16X3 / FP16X3 / FP16X3M): qkv and out point at hi planes, qkv_lo / out_lo are the ELEMENT offsets of the lo planes
 * (>= the hi plane's size, multiples of 8), terms = 3 (window_attn_pipe_kernel) or 1 (kh.qh and vh.ph alone:
 * window_attn_split_kernel); terms = 3 | 0x100 runs window_attn_split_kernel with three terms. The other compute_dtypes
 * take qkv_lo = out_lo = 0 and terms = 1. Buffers are 16-byte aligned. MNX_ERR_INVALID_ARG (with mnx_last_error) for any
 * other shape, offset or dtype / terms combination. Asynchronous on `stream`. */
int mnx_window_attn(mnx_engine* h, const void* qkv, int64_t qkv_lo, const float* table, void* out, int64_t out_lo,
                    int32_t B, int32_t H, int32_t W, int32_t C, int32_t heads, int32_t shift, int32_t terms, void* stream);

/* Test aid: copy one raw block of the decoder's K / V cache (24-bit block fixed point, molnextr_amd/csrc/kvq.h) into the
 * device buffer dst: which = 0 self-attention keys, 1 self-attention values, 2 memory keys, 3 memory values; layer
 * 0..dec_layers-1, head 0..dec_heads-1; owner = the slot (0..dec_slots-1) of a self block or the memory block of a memory
 * one. A block is the nk rows of one (owner, layer, head), nk = (max_len + 3) & ~3 for self blocks and (S + 3) & ~3 for
 * memory blocks (S = 144 memory positions): nk * 100 bytes, laid out as [nk][32] int16 hi | [nk][32] uint8 lo | [nk]
 * float scale; row j holds q = hi * 256 + lo and the value q * scale. After mnx_decode_greedy / mnx_decode_forced, row b
 * of the call used slot b (its key t at row t) and memory block b. Out-of-range arguments return MNX_ERR_INVALID_ARG
 * (with mnx_last_error). Asynchronous on `stream`. */
int mnx_kv_block(mnx_engine* h, int32_t which, int32_t layer, int32_t owner, int32_t head, void* dst, void* stream);

/* Test aid: the beam-search strategy kernels (begin, pick, gather) on scripted log-probs, without a decoder. table is device
 * fp32 [max_len][B][beam][V]: the log-prob row that hypothesis j of ORIGINAL image b sees at step t lies at
 * ((t * B + b) * beam + j) * V, whichever images have left the batch by then. One rule of the head is applied to a row
 * and nothing else: at step 0 the eos column is read as -1e20 (min_length = 1); there is no grammar mask. V = 2..256
 * stands in for the vocabulary and eos = 0..V-1 for its id; B <= 32, 1 <= n_best <= beam <= 8, 1 <= max_len <=
 * cfg.max_len, B x beam <= dec_slots. The steps run as those of mnx_decode_beam do (no graph), until no image is alive.
 * Outputs: tokens [B,n_best,max_len], lengths [B,n_best], scores [B,n_best] (device) as mnx_decode_beam gives them;
 * *steps_run (HOST): the steps that found an image alive. Trace (device; all five pointers set, or all null), row (t, b)
 * written at step t for every image b alive at the START of the step, all other rows left as the caller filled them:
 * tr_parent / tr_token / tr_score [max_len][B][beam] — of every new hypothesis the parent 0..beam-1, the id and the fp32
 * score the pick kernel ranked it by (its own word, (log-prob + cumulative) / (t + 2)); tr_alive [max_len][B] — 1 while the
 * image stays in the batch after the step; tr_n_active [max_len] — the rows (alive images x beam) the begin kernel counted,
 * written for the steps_run steps. MNX_ERR_INVALID_ARG (with mnx_last_error, "mnx_beam_scripted: ...") for anything else.
 * Synchronises `stream` before it returns. */
int mnx_beam_scripted(mnx_engine* h, const float* table, int32_t B, int32_t beam, int32_t n_best, int32_t max_len, int32_t V,
                      int32_t eos, int32_t* tokens, int32_t* lengths, float* scores, int32_t* steps_run, int32_t* tr_parent,
                      int32_t* tr_token, float* tr_score, int32_t* tr_alive, int32_t* tr_n_active, void* stream);

/* Test aid: mnx_decode_beam with the CHOICE of every step read from a script, the real decoder running underneath — teacher
 * forcing of beam search, so that a hypothesis' keys and values can be sent through any sequence of ancestor slots and the
 * logits compared step by step (a free-running search cannot be: its ranked candidates come within fp32 noise of each other).
 * features, B, beam, n_best, max_len, tokens, lengths, scores, hidden: as mnx_decode_beam (hidden may be null).
 * script_parent, script_token: HOST int32 [max_len][B][beam], script_len elements each (>= max_len x B x beam): new hypothesis
 * j of ORIGINAL image b at step t descends from hypothesis script_parent (0..beam-1) and emits id script_token
 * (0..vocab-1). The script replaces the pick kernel's K arg-max rounds and nothing else: the score of a new hypothesis is the
 * kernel's own expression for that candidate ((masked log-prob in the parent's row + the parent's cumulative) / (t + 2)), and
 * ancestry, finishing on <eos> or max_len, the pool of finished hypotheses, an image leaving and the gathers of ids and hidden
 * rows run as in mnx_decode_beam. Entries of an image that has left are validated and not read.
 * A script may not do what a top-K cannot: emit <eos> (2) at step 0, where the head bans it; descend from a hypothesis that
 * has finished; make the same (parent, token) choice twice for one image at one step. The library does not check these
 * three (the result is then not a beam search's); Engine.decode_beam_forced does. As in mnx_decode_beam only hypothesis 0
 * of an image starts with a cumulative log-prob of 0, the others with -inf: descendants of those score -inf.
 * logits_trace (may be null): device fp32 [max_len][B x beam][V], the raw logits of slot b * beam + j at step t, written for
 * the slots alive at that step; every other row is left as the caller filled it.
 * Every element of the script and every size is checked before anything is launched, and the checked copy is what the
 * device reads: MNX_ERR_INVALID_ARG (with mnx_last_error, "mnx_decode_beam_forced: ...") for a null pointer (but hidden,
 * logits_trace), B outside 1..32, beam outside 1..8, n_best outside 1..beam, max_len outside 1..cfg.max_len, B x beam >
 * dec_slots, script_len too small, a parent or an id out of range. Synchronises `stream` before it returns. */
int mnx_decode_beam_forced(mnx_engine* h, const float* features, int32_t B, int32_t beam, int32_t n_best, int32_t max_len,
                           const int32_t* script_parent, const int32_t* script_token, int64_t script_len, int32_t* tokens,
                           int32_t* lengths, float* scores, float* hidden, float* logits_trace, void* stream);

/* Test aid: mnx_edges with one more output. After the same four launches it copies, device to device on `stream`, what
 * the bond head's pair kernel left behind: probs device fp32 [B,kmax,kmax,8], laid out by the call's kmax; slots 0..6 of
 * pair (i, j) are the softmax over the 7 bond classes (before get_edge_prediction) for i, j < n_atoms[b] (clamped as
 * above). Slot 7 and every other pair are undefined. Arguments, clamping and errors as mnx_edges ("mnx_edge_probs: ...");
 * a refused call launches and copies nothing. Asynchronous on `stream`. */
int mnx_edge_probs(mnx_engine* h, const float* hidden, const int32_t* atom_idx, const int32_t* n_atoms, int32_t B,
                   int32_t kmax, int32_t max_len, uint8_t* edges, double* scores, float* probs, void* stream);

/* Test aids: the encoder's non-GEMM kernels and the decoder's fp32 SGEMM on caller device buffers
 * (tests/test_gpu_encoder_ops.py). None uses anything of the engine but its device and, where stated, its compute_dtype
 * (FP16X3M counts as FP16X3). Every fp32 buffer is 16-byte aligned, a 16-bit output 8-byte. Each returns
 * MNX_ERR_INVALID_ARG (with mnx_last_error, "mnx_<name>: ...") for a null or misaligned pointer or any size outside what
 * is stated, and launches nothing then. Asynchronous on `stream`.
 *
 * mnx_patch_embed: Conv2d(3, C, 4, stride 4) + bias + LayerNorm(C, eps 1e-5) of B images -> x fp32 [B, (S/4)^2, C].
 *   img: img_format MNX_IMG_F32 fp32 [B,3,S,S]; MNX_IMG_GRAY8 uint8 [B,S,S] (4-byte aligned), expanded to the three
 *   normalised channels as mnx_encode_gray8 does — bit-identical tokens. w_t: the conv weight as [48][C], row
 *   (ci * 4 + ky) * 4 + kx (the layout mnx_create uploads). C = 32, 64, 96 or 128; S a multiple of 4; B <= 65535. */
int mnx_patch_embed(mnx_engine* h, const void* img, int32_t img_format, const float* w_t, const float* bias,
                    const float* gamma, const float* beta, float* x, int32_t B, int32_t S, int32_t C, void* stream);

/* mnx_layernorm16: LayerNorm over the C channels of x fp32 [M, C] (C a multiple of 4, 4..2048) -> y16 [M, C] in the
 *   engine's operand type (FP32 engines: fp32) and / or y32 fp32 [M, C]; one of the two may be null. Split compute_dtypes:
 *   y16 is the hi plane, the lo plane = RN16(value - hi) lies y_lo ELEMENTS behind it (>= M * C, a multiple of 8);
 *   planes = 1 writes the hi plane only (y_lo is ignored). The other compute_dtypes take y_lo = 0 and planes = 2.
 *   flag: device int32 or null; set to 1 (never cleared) when a row's variance is not finite and positive.
 * mnx_merge_ln16: the patch-merging gather + LayerNorm(4C): x fp32 [B,H,W,C] (H, W even; C a multiple of 4, <= 512)
 *   -> y16 [B * H/2 * W/2, 4C], row (b, i, j) = LayerNorm(concat of x[b, 2i+dy, 2j+dx, :], (dy,dx) = (0,0), (1,0), (0,1),
 *   (1,1)). y_lo / planes as above. */
int mnx_layernorm16(mnx_engine* h, const float* x, const float* gamma, const float* beta, void* y16, int64_t y_lo,
                    float* y32, int32_t M, int32_t C, float eps, int32_t planes, int32_t* flag, void* stream);
int mnx_merge_ln16(mnx_engine* h, const float* x, const float* gamma, const float* beta, void* y16, int64_t y_lo,
                   int32_t B, int32_t H, int32_t W, int32_t C, float eps, int32_t planes, void* stream);

/* mnx_cast16: x fp32 [n] (n a multiple of 4) -> y16 [n] in the engine's operand type (FP32 engines: a copy). Split
 *   compute_dtypes: hi = RN16(scale * x), lo = RN16(scale * x - hi) y_lo >= n ELEMENTS (a multiple of 4) behind; scale is
 *   meant to be a power of two. The other compute_dtypes take y_lo = 0 and IGNORE scale, as the kernel does. */
int mnx_cast16(mnx_engine* h, const float* x, void* y16, int64_t y_lo, int64_t n, float scale, void* stream);

/* mnx_sgemm_tn: the decoder's fp32 SGEMM C[M,N] = A[M,K] . W[N,K]^T + bias (bias fp32 [N] or null); K a multiple of 16,
 *   N of 4. perm_S > 0 (N a multiple of 256, M of perm_S): element (m, n) is stored at
 *   [m / perm_S][n / 256][(n % 256) / 32][m % perm_S][n % 32] — the projected memory K / V layout
 *   [image][layer * 2 + K|V][head][position][32]. Independent of the compute_dtype. */
int mnx_sgemm_tn(mnx_engine* h, const float* A, const float* W, const float* bias, float* C, int32_t M, int32_t N,
                 int32_t K, int32_t perm_S, void* stream);

/* Test aid: ONE launch of one linear of the 8-launches-per-layer decode tick (mnx::dec_linear_kernel<pro, epi>,
 * molnextr_amd/csrc/decoder.hip) on caller device buffers, under a scripted tick state (tests/test_gpu_dec_linear.py).
 *   out[r, n] = epi( pro(in)[r, :] . W[n, :] + bias[n] )      for the rows r < n_alive of `capacity` launched rows
 * pro: 0 the input as it is | 1 LayerNorm(gamma, beta, eps 1e-6) of `in` — with part != null of
 *      (((p0 + p1) + ...) + p[n_part-1]) + in, p_z = part + z * part_stride, and that sum is also written to x_write
 *      [capacity, 256] | 2 LayerNorm of emb[prev_tok] * 16 + pe[rank] (the engine's tables; `in` is not read), which is
 *      also written to x_write.
 * epi: 0 N = 768: columns 0..255 * 32^-1/2 -> out [capacity, 256]; columns 256..511 / 512..767 are quantised into row t of
 *      the slot's eight key / value blocks of the engine's LAYER-0 self cache (read them with mnx_kv_block) |
 *      1 out [capacity, N] += result (in place) | 2 result * 32^-1/2 | 3 erf-GELU(result) |
 *      4 K-slice partial sums: plane z = out + z * part_stride holds the products over k in [256 z, 256 z + 256), the bias
 *      in plane 0 alone (K / 256 planes).
 * Only the six pairs the tick uses exist: (2,0), (1,0), (0,1), (1,2), (1,3), (0,4).
 * in [capacity, K], W [N, K], bias [N], gamma / beta [K]: device fp32, 16-byte aligned. N a multiple of 32, K of 256;
 * K = 256 unless pro = 0; capacity a multiple of 32, at most dec_slots; 1 <= n_alive <= capacity.
 * rows: HOST int32 [n_alive][4] = {slot, t, prev_tok, rowc} of every alive sequence, all of one reference batch: slots
 * distinct in 0..dec_slots-1 (in any order, with gaps), t < max_len, prev_tok < vocab, rowc < 512 (distinct rowc give
 * distinct PE ranks). The call resets the decoder state, installs these rows, runs the production begin kernel over all
 * dec_slots — row r of every buffer is the alive slot with the r-th smallest slot NUMBER, its PE rank the number of alive
 * rows with a smaller rowc —, launches the linear and resets the state again. Rows n_alive..capacity-1 are idle: the
 * kernel may read them and stores nothing for them, nor to any cache block.
 * MNX_ERR_INVALID_ARG (with mnx_last_error, "mnx_dec_linear: ...") for a null or misaligned pointer, another (pro, epi), or
 * any size or script entry outside what is stated; nothing is launched then. Overwrites the decoder state: not to be
 * called while a decode call is in flight. Synchronises `stream` before it returns. */
int mnx_dec_linear(mnx_engine* h, int32_t pro, int32_t epi, const float* in, const float* W, const float* bias,
                   const float* gamma, const float* beta, const float* part, int32_t n_part, int32_t part_stride, float* out,
                   float* x_write, int32_t N, int32_t K, int32_t capacity, int32_t n_alive, const int32_t* rows, void* stream);

/* Measurement aid for bench.py: while enabled, mnx_encode brackets every kernel launch of the sampled calls with a
 * pair of HIP events recorded on the stream the kernel is launched on (also inside mnx_predict, i.e. live in a timed
 * region). `enable` = n > 0: every n-th mnx_encode call since the enable is sampled, at most 4 calls (the event pool
 * stays small and is reused; the launches of the other calls run un-bracketed). mnx_profile_read synchronises and
 * returns, for one kernel class, the totals accumulated since the last reset: summed event-to-event milliseconds,
 * algorithmic work and launch count.
 *   kind 0  MFMA GEMM             work = FLOP (2*M*N*K per launch): stages with C < 512 and the patch-merging reductions
 *   kind 4  MFMA GEMM             the same for the block Linears with C >= 512 (Swin-B stages 3 and 4: the MFMA-bound shapes)
 *   kind 1  LayerNorm             work = HBM bytes (fp32 in, operand-type out [+ fp32 out])
 *   kind 2  window attention      work = HBM bytes (qkv in, context out)
 *   kind 3  patch embedding       work = HBM bytes (image in, fp32 tokens out)
 *   kind < 0  reset the pool */
int mnx_profile_enable(mnx_engine* h, int32_t enable);
int mnx_profile_read(mnx_engine* h, int32_t kind, double* ms, double* work, int64_t* launches);

/* Measurement aid: the two attention launches of a decode layer (mnx::dec_attn_kernel over the self K/V cache, and over
 * the projected memory K/V) launched `iters` times each between HIP events with `rows` sequences resident at position t.
 * Launch i reads the K/V of layer i % dec_layers, exactly as the launches of a real tick do, so that one cycle touches
 * more bytes than the 256 MB Infinity Cache holds and the time per launch is an HBM figure. Isolated (nothing else
 * runs), so the algorithmic HBM bytes per launch are known exactly: rows*8*(t+1)*256 B (self K+V) and rows*8*144*256 B
 * (cross K+V). Overwrites the decoder state: not to be called while a decode call is in flight. */
int mnx_probe_decode_attn(mnx_engine* h, int32_t rows, int32_t t, int32_t iters, double* self_ms, double* cross_ms,
                          void* stream);

/* Measurement aids (ABI 6): the encoder GEMMs are POWER-limited on this chip — the shader clock under the split-operand GEMM
 * kernel is 1.65-1.9 GHz with real operands against 2.4 GHz nominal — so a rate is reported next to the clock it
 * was reached at and next to what the matrix pipes sustain on this device.
 * mnx_gemm_clock: shader clock (MHz; shader cycles / 100 MHz wall ticks of one workgroup per launch) averaged over the persistent
 *   GEMM launches (mnx::gemm256x3_kernel) since the last reset; 0.0 when none ran. Synchronises the device. The counters are
 *   per process (all engines of the device share them).
 * mnx_probe_mfma: runs a register-only loop of v_mfma_f32_16x16x32_f16 on random operands on every CU for about ms_target
 *   milliseconds (after a shorter settling launch) and returns its rate (TFLOP/s) and shader clock: the ceiling of any fp16
 *   MFMA kernel under this device's power budget — no reference-side counterpart (measurement only). */
int mnx_gemm_clock(mnx_engine* h, int32_t reset, double* mhz);
int mnx_probe_mfma(mnx_engine* h, int32_t ms_target, double* tflops, double* mhz, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOLNEXTR_HIP_H */
