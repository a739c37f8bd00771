/*
 * vcap.h - C ABI of the MI355X-native video-caption hot path (libvcap_hip.so).
 *
 * Plain pointers and sizes only: device pointers are HIP device addresses, `stream` is a
 * hipStream_t passed as void*.  Every entry point returns 0 on success or a negative code
 * (-hipError_t, or VCAP_E_* for argument errors) and sets a thread-local message readable
 * with vcap_last_error().  Nothing allocates device memory behind the caller's back: the
 * caller owns the workspace (size from the *_workspace_bytes queries); nothing synchronises
 * the stream.
 *
 * Reference interfaces each entry point replaces (paths relative to the reference repo):
 *   vcap_linear_bias        core/operators/cupy_linear_mapper.py:14-70 (linear_bias_f32/_f16 CUDA-C)
 *                           and CuPyLinearCompat.forward :137-184 (nn.Linear drop-in)
 *   vcap_vit_pool_temporal  core/operators/cupy_vit_pool.py:23-104 (vit_pool_{cls,gap}_{f32,f16}),
 *                           vit_fused_pool_temporal :127-186
 *   vcap_prefix_project     core/operators/normalization.py:6-13 apply_prefix_norm + the decoder
 *                           mapper (src/models/text_decoder.py:249), i.e. core/engine.py:44-50 -> :60-74
 *   vcap_gemm / vcap_layernorm / vcap_vit_attention / vcap_gemm_mx / vcap_layernorm_mx
 *                           the timm ViT block arithmetic the reference drives through
 *                           src/models/video_encoder.py:112-174 (fused SDPA, tanh-GELU MLP,
 *                           in-place residual) - op-level entry points for the plugin registry
 *                           (core/operators/trt_plugin_hooks.py:7-34)
 *   vcap_frames_preprocess  core/preprocessing/frame_loader.py:34-45 (Resize -> ToTensor -> Normalize)
 *   vcap_vit_encode         ViTFrameEncoder.forward (src/models/video_encoder.py:288-326) fused with
 *                           the engine prefix (core/engine.py:43-50) and the mapper
 *   vcap_gpt2_generate      GPT2TextDecoder.generate (src/models/text_decoder.py:105-146) ->
 *                           GPT2LMHeadModel.generate greedy with RepetitionPenalty / NoRepeatNGram /
 *                           MinNewTokens, and the raw greedy loop of
 *                           core/scripts/benchmark_baseline.py:160-240 (processors disabled)
 *   vcap_l2_normalize       F.normalize of ViTTextAlignModel.encode_video (src/models/vit_text_align.py:54-65)
 *                           and ViTFrameEncoder l2norm (src/models/video_encoder.py:318-319); the l2norm
 *                           helper of scripts/query_video.py:20-21
 *   vcap_ip_index_convert / vcap_ip_search
 *                           faiss.normalize_L2 + IndexFlatIP.add (scripts/build_index.py:40-42) and
 *                           index.search (scripts/query_video.py:61-75, 127)
 *   vcap_ivf_assign / vcap_ivf_centroid_update / vcap_ivf_search
 *                           faiss.IndexIVFFlat train / add / search with METRIC_INNER_PRODUCT
 *                           (build_faiss of scripts/build_index_with_captions.py:33-45)
 *   vcap_text_encode        ViTTextAlignModel.encode_text (src/models/vit_text_align.py:67-79)
 *   vcap_vit_encode_backward / vcap_vit_attention_backward
 *                           loss.backward() through ViTTextAlignModel.encode_video's ViT with freeze_vit
 *                           off (src/cli/train_full.py:47, :124-130: AdamW over model.parameters()); the
 *                           optimiser itself stays in torch
 */
#ifndef VCAP_H_
#define VCAP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VCAP_ABI_VERSION 16

/* VCAP_DT_MXFP8: OCP e4m3fn elements + one E8M0 scale per 32 consecutive K elements of a row
 * (the gfx950 block-scaled MFMA format; BASELINE configs[4]).  Scale arrays use the GEMM's
 * staging order: per (128-wide K-tile, group of 256 rows) one 1 KiB block laid out
 * [k-block 0..3][row % 16][row / 16] - byte offset
 *   ((k/128 * ceil(rows/256) + row/256) * 4 + (k%128)/32) * 256 + (row%16) * 16 + (row%256)/16,
 * size vcap_mx_scale_bytes(rows, K).  Element value = e4m3 * 2^(scale - 127).
 * VCAP_DT_F16: IEEE binary16 (torch.float16), the dtype of the reference's ViT autocast
 * (src/models/video_encoder.py:261-264).  A ViT operand format only: vcap_vit_desc.dtype, vcap_gemm,
 * vcap_linear_bias, vcap_layernorm, vcap_vit_attention, vcap_vit_qkv_attention_dt and
 * vcap_vit_pool_temporal take it; the decoder (vcap_gpt2_*, vcap_rows_pack*, vcap_decode_attention)
 * and the MXFP8 entry points refuse it.  With F16 operands a GEMM rounds where autocast does: the
 * accumulator + bias to fp16 before an f32 residual / positional add, and the GELU's input and
 * output to fp16; conversions round to nearest even, overflow to +-inf, subnormals kept. */
enum { VCAP_DT_F32 = 0, VCAP_DT_BF16 = 1, VCAP_DT_MXFP8 = 2, VCAP_DT_F16 = 3 };
enum { VCAP_E_ARG = -1000, VCAP_E_WORKSPACE = -1001, VCAP_E_UNSUPPORTED = -1002 };

typedef struct vcap_vit_layer {
  const float* ln1_g; const float* ln1_b;
  const void* qkv_w; const float* qkv_b;     /* [3D, D] */
  const void* proj_w; const float* proj_b;   /* [D, D]  */
  const float* ln2_g; const float* ln2_b;
  const void* fc1_w; const float* fc1_b;     /* [4D, D] */
  const void* fc2_w; const float* fc2_b;     /* [D, 4D] */
  /* dtype VCAP_DT_MXFP8 only: qkv_w / proj_w / fc1_w / fc2_w are e4m3 and these their E8M0
   * scales (vcap_mx_quantize); the patch-embed weight stays bf16 */
  const uint8_t* qkv_ws; const uint8_t* proj_ws; const uint8_t* fc1_ws; const uint8_t* fc2_ws;
} vcap_vit_layer;

typedef struct vcap_vit_desc {
  int dtype;                 /* operand dtype of the block GEMMs (VCAP_DT_*; F16: weights fp16, workspace
                                as BF16's, autocast's rounding points; MXFP8: QKV / attn-proj /
                                fc1 / fc2 in MXFP8 with LayerNorm, attention and GELU emitting MXFP8
                                operands; patch-embed and the QK^T / PV products in bf16) */
  int dim, depth, heads, patch, image, mlp, video_dim;
  int kpad;                  /* patch K (3*p*p) padded to the GEMM K step */
  float ln_eps;              /* 1e-6 (timm) */
  const void* patch_w;       /* [dim, kpad] */
  const float* patch_b;      /* [dim] */
  const float* cls;          /* [dim] */
  const float* pos;          /* [tokens, dim] */
  const float* norm_g; const float* norm_b;
  const float* proj_w;       /* encoder.proj [video_dim, dim] f32 */
  const float* proj_b;
  const vcap_vit_layer* layers;  /* host array of `depth` entries */
} vcap_vit_desc;

typedef struct vcap_prefix_desc {
  float ln_scale;            /* <=0 disables the layer_norm*ln_scale step (core/engine.py:47) */
  float in_weight;           /* <=0 disables the *in_weight step (core/engine.py:49) */
  int prefix_len, n_embd;
  const float* mapper_w;     /* [prefix_len*n_embd, video_dim] f32 */
  const float* mapper_b;
} vcap_prefix_desc;

/* GPT-2 projection weights are passed ROWS-PACKED: the torch Linear-layout [N, K] matrix
 * (Conv1D weights transposed) rearranged by vcap_rows_pack() into MFMA-fragment order, so each
 * decode weight load is one contiguous 1 KiB wave instruction (layout in csrc/decode.hip). */
typedef struct vcap_gpt2_layer {
  const float* ln1_g; const float* ln1_b;
  const void* attn_w; const float* attn_b;   /* packed [3E, E] (c_attn Conv1D transposed) */
  const void* aproj_w; const float* aproj_b; /* packed [E, E] */
  const float* ln2_g; const float* ln2_b;
  const void* fc_w; const float* fc_b;       /* packed [4E, E] */
  const void* mproj_w; const float* mproj_b; /* packed [E, 4E] */
} vcap_gpt2_layer;

/* Widths: n_embd any multiple of 128 up to 1024 with n_head = n_embd / 64, in both dtypes.  The mlp
 * c_proj (K = 4 * n_embd) splits its K range over workgroups only where a kernel implements it: bf16
 * at K = 3072; f32 at K / 64 = 48 or 64 slabs (K = 3072 / 4096) with one 16-column tile per workgroup.
 * Every other width and grid cap runs that projection unsplit (csrc/decode.hip
 * vcap_rows_gemm_dispatch; DESIGN.md "Decoder widths"). */
typedef struct vcap_gpt2_desc {
  int dtype;
  int n_embd, n_layer, n_head, vocab, n_positions, prefix_len;
  float ln_eps;              /* 1e-5 */
  const void* wte;           /* [vocab, E] token embedding (plain layout, row gathers) */
  const void* lm_head;       /* packed [vocab, E]: the tied lm_head = vcap_rows_pack(wte) */
  const float* wpe;          /* [n_positions, E] f32 */
  const float* lnf_g; const float* lnf_b;
  const vcap_gpt2_layer* layers; /* host array of n_layer entries */
  /* f32 decoders, optional (NULL / 0 disable): a bf16 rows-packed copy of the lm_head and
   * screen_bound = c * max_v ||w_v||_2 with c >= 2u + u^2 + 4 * 1024 * 2^-24 = 8.07e-3 (u = 2^-8, the
   * bf16 unit roundoff of EACH of h and w; the two f32 dot products over n_embd <= 1024, doubled
   * for a truncating accumulator; vcap/model.py uses c = 0.0082).  The runtime scales the bound by
   * max(rep, 1/rep) while a repetition penalty is active.  A greedy step without requested logits then runs the
   * lm_head in bf16 as a screen and rescores, in f32 against wte, every token whose exact score
   * could reach the screen's maximum: the token is the exact f32 argmax (processors applied, ties
   * to the lowest id) at half the lm_head's weight bytes. */
  const void* lm_head_screen;
  float screen_bound;
} vcap_gpt2_desc;

typedef struct vcap_gen_params {
  int max_new_tokens;
  int min_new_tokens;        /* 0 for raw greedy */
  int no_repeat_ngram_size;  /* 0 disables */
  float repetition_penalty;  /* 1.0 disables */
  int eos_token_id, pad_token_id;
  int use_graph;             /* capture the whole decode into a hipGraph and replay it */
  int max_blocks;            /* 0: whole-chip grids; > 0: cap the projection GEMV grids near this
                                many workgroups (wider tiles per workgroup) - for a decode that
                                shares the GPU with an encode holding most CUs */
} vcap_gen_params;

const char* vcap_last_error(void);
int vcap_abi_version(void);

/* ---- tuning: which ViT GEMM kernel vcap_gemm / vcap_vit_encode use (process-wide):
 *      0 auto (256x256-tile kernel when the shape yields >= 512 tiles), 1 128x128 only,
 *      2 256x256 wherever its shape constraints hold.  Results are identical up to fp32
 *      summation order within a tile (both accumulate K in the same order). ---- */
int vcap_set_gemm_policy(int policy);

/* ---- a stream whose kernels avoid `reserve_cus` CUs (hipExtStreamCreateWithCUMask), so a
 *      latency-bound chain on another stream (the decode graph) always finds free CUs while
 *      the MFMA-bound encode fills the rest.  Destroy with vcap_stream_destroy. ---- */
int vcap_stream_create_cu_reserved(int reserve_cus, void** stream);
int vcap_stream_create_cu_mask(const uint32_t* mask, int words, void** stream);  /* raw CU bit mask */
int vcap_stream_destroy(void* stream);

/* ---- op-level entry points ---- */
int vcap_linear_bias(int dtype, const void* x, const void* w, const float* b, void* y, int rows, int in_features,
                     int out_features, void* stream);
/* C[orow(m)][n] = epilogue(sum_k A[m][k] W[n][k]): F32, BF16 or F16 operands, K a multiple of one 128-byte K-tile
 * row.  Both kernels fetch the operands by 16-byte LDS-DMA, so A and W must be 16-byte aligned and lda, ldw whole
 * 16-byte vectors (4 f32 / 8 bf16 or f16 elements); anything else is VCAP_E_UNSUPPORTED before any launch
 * (vcap_gemm_splitk alike).  The 256x256-tile kernel is not used when (M - 1) * lda or (N - 1) * ldw reaches
 * 2^32 bytes (its operand offsets are 32-bit): such a call runs the 128x128-tile kernel under every policy.
 * C, bias and res need only their element's alignment: the epilogues reach them with plain global vector loads
 * and stores, which rely on the device's unaligned access mode (the HSA default) below 16 bytes.  BF16 operands
 * write BF16 or F32, F16 operands F16 or F32, F32 operands F32; another pair is VCAP_E_UNSUPPORTED. */
int vcap_gemm(int in_dtype, int out_dtype, const void* A, int64_t lda, const void* W, int64_t ldw, void* C,
              int64_t ldc, int M, int N, int K, const float* bias, int act, const float* res, int64_t ldr,
              int res_mode, int G, int Gs, int goff, int roff, void* stream);
/* The in-place residual GEMM of the encoder's class-token-only last block, at the op level:
 *   C[orow(m)][n] += sum_k A[m][k] W[n][k] + bias[n],   orow(m) = G ? (m / G) * Gs + m % G : m
 * with BF16 or F16 operands, f32 C, and a caller workspace (>= 8 * M * N * 4 bytes, 16-byte aligned) for
 * deterministic split-K partials: K is split over the largest c <= 8 dividing the K-tile count with >= 3
 * K-tiles per split (a launch that splits runs the 128x128 kernel under every gemm policy and tile count:
 * the split count depends on K alone), the
 * partial slabs are summed in split order by a second kernel, and - F16 - the sum + bias is rounded to
 * fp16 there, before the add.  *splits_out (optional) receives c (1: not split).  This is the path
 * vcap_vit_encode takes for attn-proj / fc2 of its last block. */
int vcap_gemm_splitk(int in_dtype, const void* A, int64_t lda, const void* W, int64_t ldw, float* C, int64_t ldc,
                     int M, int N, int K, const float* bias, int G, int Gs, void* workspace, size_t ws_bytes,
                     int* splits_out, void* stream);
int vcap_layernorm(int out_dtype, const float* x, int64_t ldx, void* y, int64_t ldy, const float* gamma,
                   const float* beta, int rows, int dim, float eps, void* stream);
int vcap_vit_attention(int dtype, const void* qkv, void* out, int frames, int tokens, int heads, void* stream);
/* Fused QKV projection + attention (bf16; 192 < tokens <= 208 or 256 < tokens <= 272, i.e. ViT-B/16
 * and ViT-L/14 frames): xn
 * [frames*tokens, heads*64] bf16 (the LayerNorm output), wqkv [3*heads*64, heads*64] bf16, bqkv
 * [3*heads*64] f32 -> out [frames*tokens, heads*64] bf16 (cls_only: [frames, heads*64], the class
 * token's row).  Bit-identical to vcap_gemm (bias, bf16 out) into a qkv buffer followed by
 * vcap_vit_attention; q / k / v stay on chip.  Replaces timm Attention.qkv + the attention core
 * (src/models/video_encoder.py:112-121).  VCAP_E_UNSUPPORTED outside that shape. */
int vcap_vit_qkv_attention(const void* xn, const void* wqkv, const float* bqkv, void* out, int frames, int tokens,
                           int heads, int cls_only, void* stream);
/* The same with the 2-byte element type chosen: dtype VCAP_DT_BF16 (= vcap_vit_qkv_attention) or
 * VCAP_DT_F16 (xn, wqkv and out fp16; bit-identical to the F16 vcap_gemm + vcap_vit_attention pair). */
int vcap_vit_qkv_attention_dt(int dtype, const void* xn, const void* wqkv, const float* bqkv, void* out, int frames,
                              int tokens, int heads, int cls_only, void* stream);

/* ---- frame preprocessing (core/preprocessing/frame_loader.py:34-45: torchvision Resize((S, S)) on
 *      PIL images -> ToTensor -> Normalize): decoded RGB frames uint8 [n, in_h, in_w, 3] (device)
 *      -> out f32 [n, 3, out_h, out_w] (normalised) and/or out_u8 [n, out_h, out_w, 3] (the resized
 *      pixels), bit-identical to PIL Image.resize(BILINEAR) + the f32 /255, -mean, /std chain.
 *      mean3 / std3 are HOST arrays of 3 floats.  Downscale factors up to 31. ---- */
size_t vcap_frames_workspace_bytes(int n, int in_h, int in_w, int out_h, int out_w);
int vcap_frames_preprocess(const uint8_t* frames, int n, int in_h, int in_w, int out_h, int out_w, const float* mean3,
                           const float* std3, float* out, uint8_t* out_u8, void* workspace, size_t ws_bytes,
                           void* stream);

/* ---- JPEG frame decode (core/preprocessing/frame_loader.py:42-44: PIL Image.open(path).convert("RGB"),
 *      i.e. libjpeg-turbo's default decompression) for baseline sequential Huffman JPEGs: 8-bit, 1 or
 *      3 components in one interleaved scan, 4:4:4 / 4:2:2 / 4:2:0, restart markers.  The host
 *      parses and entropy-decodes (parallel threads, one image each); the device dequantises and runs
 *      jpeg_idct_islow, fancy-upsamples chroma and converts YCbCr -> RGB with libjpeg's fixed-point
 *      arithmetic: bit-identical to libjpeg's C decoder (jidctint.c, jdsample.c, jdcolor.c) for every
 *      accepted stream, and to Pillow's default decode (libjpeg-turbo's SIMD IDCT) while no IDCT output
 *      leaves [-512, 511] before the level shift - four times what real pixels give; beyond it the C code
 *      wraps through its range table and the SIMD code saturates (DESIGN.md "JPEG decode sweep").  16-bit
 *      DQT entries multiply as signed 16-bit values, as libjpeg-turbo holds them.  A chroma plane whose
 *      downsampled width is 2 or less is refused.  Progressive / arithmetic-coded / 12-bit / CMYK images ->
 *      VCAP_E_UNSUPPORTED, and so are RGB-coded JPEGs (libjpeg's colour-space rule: no JFIF marker and
 *      an Adobe transform of 0, or component ids 'R','G','B').  vcap_jpeg_decode_batch: n images (HOST
 *      byte buffers) that share size and chroma sampling (each image keeps its own quantisation and
 *      Huffman tables, as ffmpeg's per-frame MJPEG qscale writes them) -> out uint8 [n, H, W, 3]
 *      (device); returns after the device work of the call has finished, on every path (the host
 *      coefficient staging is released). ---- */
int vcap_jpeg_probe(const uint8_t* data, size_t len, int* width, int* height, int* comps);
size_t vcap_jpeg_workspace_bytes(const uint8_t* data, size_t len, int n);
int vcap_jpeg_decode_batch(const uint8_t* const* data, const size_t* lens, int n, uint8_t* out, void* workspace,
                           size_t ws_bytes, void* stream);

/* ---- MXFP8 (BASELINE configs[4]: fp8 MFMA path for the ViT GEMMs) ----
 * vcap_mx_quantize: rows of f32 / bf16 [rows, K] (row stride ldx) -> e4m3 [rows, K] + scales.
 *   Per block of 32: scale byte max(exponent field of max|x| - 7, 0), i.e. 2^(floor(log2 max|x|) - 7)
 *   clamped at 2^-127 (a block max below 2^-120, f32 subnormals and an all-zero block give byte 0);
 *   elements x * 2^(127 - scale) rounded to nearest even, |scaled| <= 256, so nothing saturates; -0.0
 *   stays -0.0 (0x80).  Writes rows * K bytes of q and the scale bytes of rows 0..rows-1 only (the
 *   padding rows of the last 256-row group are left as they were).
 *   Non-finite input (tests/test_gpu_mx_sweep.py): other blocks are unaffected.  A NaN takes no part in
 *   its block's max (fmaxf), so the block's scale and its finite elements are those of the block without
 *   it, and the NaN is stored as an e4m3 NaN (0x7F / 0xFF).  A block holding +-inf gets scale byte 248:
 *   its finite elements are scaled by 2^-121 (FLT_MAX -> 128; every |x| below 2^111 has a scaled value
 *   below 2^-10, half the smallest e4m3 subnormal, and becomes +-0) and the
 *   infinity itself is stored as whatever the hardware converter gives an overflow - an e4m3 NaN or
 *   +-448 - the same byte on every run; callers must not rely on which.
 * vcap_layernorm_mx: LayerNorm (f32 rows) fused with the quantisation of its output (same rule).
 * vcap_gemm_mx: C = epi(A . W^T) with A [M, K], W [N, K] MXFP8 (contiguous rows, K % 256 == 0);
 *   out_dtype BF16 / F32 (res != NULL, f32 only: C = res + ..., res read with C's row stride ldc; res == C
 *   is the in-place residual add) or MXFP8 (act must be 1 = bias +
 *   GELU-tanh, C e4m3 [M, N] + c_scales (8-byte aligned, vcap_mx_scale_bytes(M, N) bytes: the
 *   padding rows of the last 256-row group are written too), N % 128 == 0).  N and ldc are multiples
 *   of 16; rows >= M and columns [N, ldc) of C are never written. */
size_t vcap_mx_scale_bytes(int rows, int K);
/* bf16 qkv [frames*tokens, 3*heads*64] -> attention output in MXFP8 ([frames*tokens, heads*64] e4m3 +
 * scales, one per 32 of a head's 64 dims, quantised from the f32 value), the A operand of an MXFP8
 * attn-proj GEMM.  Serves 1..32, 193..224 and 257..288 tokens and heads*64 % 256 == 0; anything else is
 * VCAP_E_UNSUPPORTED before any launch. */
int vcap_vit_attention_mx(const void* qkv, void* out, uint8_t* out_scales, int frames, int tokens, int heads,
                          void* stream);
int vcap_mx_quantize(int in_dtype, const void* x, int64_t ldx, int rows, int K, void* q, uint8_t* scales,
                     void* stream);
int vcap_layernorm_mx(const float* x, int64_t ldx, void* q, uint8_t* scales, const float* gamma, const float* beta,
                      int rows, int dim, float eps, void* stream);
int vcap_gemm_mx(const void* A, const uint8_t* a_scales, const void* W, const uint8_t* w_scales, int out_dtype,
                 void* C, int64_t ldc, uint8_t* c_scales, int M, int N, int K, const float* bias, int act,
                 const float* res, void* stream);
int vcap_vit_pool_temporal(int dtype, const void* feat, void* out, int bsz, int timesteps, int tokens, int channels,
                           int pool_gap, void* stream);
int vcap_prefix_project(const float* emb, int B, int video_dim, const vcap_prefix_desc* pd, float* prefix_out,
                        void* stream);

/* ---- weight layout for the GPT-2 decoder (one-time, at model load) ----
 * vcap_rows_packed_bytes: bytes of the packed copy of a [N, K] matrix (N rounded up to 16).
 * vcap_rows_pack: w [N, K] row stride ldw (elements, 16-byte aligned rows) -> packed.
 * K must be a multiple of 32 (bf16) / 16 (f32); the decoder needs n_embd % 128 == 0. */
size_t vcap_rows_packed_bytes(int dtype, int N, int K);
int vcap_rows_pack(int dtype, const void* w, int64_t ldw, int N, int K, void* packed, void* stream);

/* ---- fused paths ----
 * ViT descriptor limits (VCAP_E_UNSUPPORTED before any launch, workspace query 0): head_dim 64, dim <= 1024,
 * video_dim <= 1024, dim / mlp / kpad multiples of the GEMM K step, a square grid of at most 288 tokens (class
 * token included) - 33..192 and 225..256 tokens in VCAP_DT_F16 only, the one dtype the generic attention
 * kernel is built for. */
size_t vcap_vit_workspace_bytes(const vcap_vit_desc* d, int B, int T);
int vcap_vit_encode(const vcap_vit_desc* d, const vcap_prefix_desc* pd, const float* frames, int B, int T,
                    float* enc_out, float* prefix_out, void* workspace, size_t ws_bytes, void* stream);
/* ABI v15: 1 when vcap_vit_encode runs block `layer`'s QKV projection and attention as the fused
 * vcap_vit_qkv_attention kernel, 0 when as a QKV GEMM + attention kernel (fp32 operands, MXFP8 QKV /
 * attn-proj, other token counts), < 0 on a bad descriptor / layer.  The same predicate the encode
 * uses, for callers that attribute FLOPs and bytes per kernel (bench.py). */
int vcap_vit_layer_fuses_qkv_attention(const vcap_vit_desc* d, int layer);

size_t vcap_gpt2_workspace_bytes(const vcap_gpt2_desc* d, int B, int S0, int max_new_tokens);
int vcap_gpt2_generate(const vcap_gpt2_desc* d, const vcap_gen_params* gp, const float* prefix, const int* prompt_ids,
                       int prompt_len, int B, int* out_ids, float* logits_out, void* workspace, size_t ws_bytes,
                       void* stream);
/* ---- sampling presets (core/inference.py:12-15 natural / safe_sample; HF _sample as
 *      text_decoder.py:131-144 reaches it with do_sample = num_beams == 1 and temperature != 1):
 *      the greedy decode's processors, then TemperatureLogitsWarper -> TopKLogitsWarper(top_k) ->
 *      TopPLogitsWarper(top_p) -> one multinomial draw per row and step from a counter-based
 *      Philox4x32-10 stream keyed on `seed` (csrc/sample.hip).  The same hipGraph serves every seed.
 *      warped_out (optional, [max_new][B][vocab] f32): the warped scores each draw used (-inf where
 *      removed), i.e. HF's output_scores; force_ids (optional, [B][max_new]): emit these tokens
 *      instead of drawing (tests replay a recorded history).  Parity with the reference is
 *      distributional: the RNG streams differ.
 *      The draw: u = (word 0 of Philox4x32-10(counter (step, row, 0, 0), key (seed low, seed high))
 *      >> 8) / 2^24; the kept tokens are walked ascending by score, ties by vocabulary index, and the
 *      token is the first whose cumulative exp(s - max) exceeds u * total.  A row without a finite
 *      score emits EOS without a draw.
 *      One departure from HF: top-k keeps every score tied at the k-th value, and so does HF, but
 *      the kernel holds at most 256 survivors.  A row with more (over 256 - (k - 1) scores tied at
 *      the threshold) keeps every score strictly above the threshold and then the tied tokens of
 *      lowest vocabulary index until 256 are kept; top-p and the draw run over those 256.  The
 *      result is deterministic: the same row gives the same support and the same token. ---- */
typedef struct vcap_sample_params {
  float temperature;  /* > 0 */
  int top_k;          /* HF generation-config default 50; 1..128 */
  double top_p;       /* (0, 1] */
  uint64_t seed;
} vcap_sample_params;
int vcap_gpt2_sample(const vcap_gpt2_desc* d, const vcap_gen_params* gp, const vcap_sample_params* sp,
                     const float* prefix, const int* prompt_ids, int prompt_len, int B, int* out_ids,
                     float* logits_out, float* warped_out, const int* force_ids, void* workspace, size_t ws_bytes,
                     void* stream);
void vcap_graph_cache_clear(void);
/* number of instantiated decode graphs held by the cache (bounded LRU, VCAP_GRAPH_CACHE_MAX) */
int vcap_graph_cache_size(void);
/* decoder rows one call may carry: B * (prefix + prompt) at the prefill, B * num_beams per step */
int vcap_gpt2_max_rows(void);

/* ---- causal decode attention over the paged KV cache (one GPT-2 layer; HF GPT2Attention's
 *      sdpa path at decode time, text_decoder.py:131-144 -> modeling_gpt2): q [M, H*64] (M = seqs *
 *      S_new rows), pools [pages][H][16][64], page_table [seqs][maxp] or NULL for the contiguous
 *      layout (page of position j of sequence s = s*maxp + j/16), out [M, H*64].  Row m attends
 *      to positions 0 .. past + (m % S_new) of its sequence. ---- */
int vcap_decode_attention(int dtype, const void* q, const void* k_pool, const void* v_pool, const int* page_table,
                          int maxp, void* out, int M, int heads, int S_new, int past, void* stream);

/* ---- device beam search (HF `_beam_search` as text_decoder.py:131-144 reaches it for the
 *      `precise` / `detailed` presets: log_softmax -> RepetitionPenalty -> NoRepeatNGram ->
 *      MinNewTokens -> + beam scores -> top-2*num_beams, length_penalty, early_stopping=False).
 *      The whole search (prefill + max_new steps + bookkeeping) is one call, replayed as one
 *      hipGraph; out_ids [B, max_new] = each sequence's best finished hypothesis (EOS-padded),
 *      out_len [B] = its generated length (HF returns the first max(out_len) columns).
 *      Limits: B <= 8 sequences, 2 <= num_beams <= 8, max_new <= 64, prefix+prompt+max_new <= 128. ---- */
typedef struct vcap_beam_params {
  int num_beams;
  int max_new_tokens;
  int min_new_tokens;
  int no_repeat_ngram_size;
  float repetition_penalty;
  float length_penalty;
  int early_stopping;  /* only 0 (False) */
  int eos_token_id;
  int use_graph;
  int max_blocks;      /* ABI v14: as vcap_gen_params.max_blocks - 0: whole-chip grids; > 0: cap each step's
                          projection GEMV grids and the beam lm_head's grid near this many workgroups */
} vcap_beam_params;
size_t vcap_gpt2_beam_search_workspace_bytes(const vcap_gpt2_desc* d, int B, int num_beams, int S0,
                                             int max_new_tokens);
int vcap_gpt2_beam_search(const vcap_gpt2_desc* d, const vcap_beam_params* bp, const float* prefix,
                          const int* prompt_ids, int prompt_len, int B, int* out_ids, int* out_len, void* workspace,
                          size_t ws_bytes, void* stream);

/* ---- step-wise decode for host-driven search (beam search / sampling).  One state carved for
 *      `rows` decoder rows lives in the caller's workspace across calls:
 *        prefill  B <= rows sequences into rows [0, B), logits of each last position -> [B, vocab]
 *        step     feed one token per row at position `pos` (S0 <= pos < S0+max_new) -> [rows, vocab]
 *        reorder  row r <- row src_rows[r] for cache positions [0, length)   (beam reordering,
 *                 also the B -> B*num_beams expansion after prefill) ---- */
size_t vcap_gpt2_beam_workspace_bytes(const vcap_gpt2_desc* d, int rows, int S0, int max_new_tokens);
int vcap_gpt2_prefill(const vcap_gpt2_desc* d, const float* prefix, const int* prompt_ids, int prompt_len, int B,
                      int rows, int max_new_tokens, float* logits_out, void* workspace, size_t ws_bytes, void* stream);
int vcap_gpt2_step(const vcap_gpt2_desc* d, const int* tokens, int rows, int S0, int max_new_tokens, int pos,
                   float* logits_out, void* workspace, size_t ws_bytes, void* stream);
int vcap_gpt2_reorder(const vcap_gpt2_desc* d, const int* src_rows, int rows, int S0, int max_new_tokens, int length,
                      void* workspace, size_t ws_bytes, void* stream);
/* ---- the same state driven by input EMBEDDINGS (HF `GPT2LMHeadModel(inputs_embeds=...,
 *      past_key_values=..., use_cache=True)` as core/scripts/benchmark_baseline.py:160-240 calls
 *      it through `model.decoder.model`): past_len == 0 -> prefill of n_tok == S0 positions
 *      (rows sequences, embeds [rows, S0, E] f32); past_len > 0 -> one position (n_tok == 1,
 *      embeds [rows, 1, E]) at S0 <= past_len < S0 + max_new_tokens.  h = embeds + wpe[pos];
 *      logits of each row's last position -> [rows, vocab] f32.  Same workspace as above. ---- */
int vcap_gpt2_forward_embeds(const vcap_gpt2_desc* d, const float* embeds, int rows, int n_tok, int past_len, int S0,
                             int max_new_tokens, float* logits_out, void* workspace, size_t ws_bytes, void* stream);

/* ---- teacher-forced scoring (added within ABI v16: two new symbols, nothing else changes): one forward
 *      over B sequences of S input embeddings with logits, target log-probs and the LM loss at EVERY
 *      position - GPT2TextDecoder.forward / VideoCaptionModel.forward / compute_loss of the reference
 *      (src/models/text_decoder.py:76-103, src/models/caption_model.py:83-91, 104-168), forward pass
 *      only.  All pointers are device memory.
 *        embeds      [B, S, E] f32 inputs_embeds; h = embeds + wpe[0..S): positions are 0..S-1 whatever
 *                    the mask holds, as HF's GPT2LMHeadModel(inputs_embeds=, attention_mask=) forward
 *                    does (pinned by tests/golden/score_tiny.npz, the reference's own output)
 *        key_mask    [B, S] bytes or NULL (all ones): query i of sequence b attends to the keys j <= i
 *                    with key_mask[b][j] != 0.  PRECONDITION: key_mask[b][0] != 0 (the reference always
 *                    prepends ones for the prefix, so no row is ever fully masked).  It is checked on the
 *                    device, without a host synchronisation: every logprob_out entry of an offending
 *                    sequence is NaN, and loss_out[0] with them if one of its positions is counted (callers holding the mask on the host check it
 *                    there: vcap.model.HipGPT2Decoder.score raises VCAP_E_ARG)
 *        targets     [B, S] or NULL: the token to predict AT position i (already shifted: the caller does
 *                    HF's logits[:, :-1] vs labels[:, 1:]); -100 (any value outside [0, vocab)) = ignored
 *        logits_out  [B, S, vocab] f32 or NULL (not stored then)
 *        logprob_out [B, S] f32 or NULL: log_softmax(logits[b, i])[targets[b, i]], 0 where ignored
 *        loss_out    [2] f32 or NULL: {sum of -logprob over the counted positions, their count}
 *      Limits: B * S <= vcap_gpt2_max_rows() and S <= n_positions (VCAP_E_UNSUPPORTED otherwise); both
 *      decoder dtypes.  Deterministic: fixed reduction orders, no float atomics, so two calls on the same
 *      inputs give the same bits.  The call leaves no KV state and is not graph-captured. ---- */
size_t vcap_gpt2_score_workspace_bytes(const vcap_gpt2_desc* d, int B, int S);
int vcap_gpt2_score(const vcap_gpt2_desc* d, const float* embeds, int B, int S, const uint8_t* key_mask,
                    const int* targets, float* logits_out, float* logprob_out, float* loss_out, void* workspace,
                    size_t ws_bytes, void* stream);

/* ---- the scoring call's gradient w.r.t. inputs_embeds (added within ABI v16: new symbols and two new structs,
 *      nothing existing changes): vcap_gpt2_score's forward, then an activation-only backward through the
 *      frozen GPT-2 - what fitting a prefix mapper, soft prompts or an embedding saliency needs (the
 *      reference's recipe: src/cli/train_caption_mapper.py compute_loss_local, GPT-2 and ViT frozen).  This
 *      call returns no weight gradients; vcap_gpt2_score_backward_tail below adds those of the last blocks.
 *        embeds, key_mask, targets, logprob_out, loss_out: exactly vcap_gpt2_score's, the precondition
 *                    key_mask[b][0] != 0 included; targets is required here
 *        grad_logprob [B, S] f32 or NULL: the weight w[b][i] of each counted position's log-prob lp[b][i];
 *                    NULL = -1 everywhere (the gradient of loss_out[0], the NLL sum).  Entries at ignored
 *                    positions are not read.
 *        grad_embeds [B, S, E] f32, required: sum over the counted (b, i) of w[b][i] * d lp[b][i] / d embeds.
 *                    wpe is added to the embeddings, so the gradient passes through it unchanged.  Every
 *                    entry of a sequence that breaks the mask precondition is NaN.
 *      The grad desc carries the extra weight copies the backward reads, all in the decoder dtype and plain
 *      row-major: HF's Conv1D [in, out] matrices as stored (every dx = dy . W^T is then an ordinary
 *      C[m][n] = sum_k A[m][k] W[n][k] product), the Linear-layout [out, in] copies of c_attn and c_fc for
 *      the recompute of q | k | v and of the pre-GELU c_fc output, and wte transposed with its vocabulary
 *      axis zero-padded to a multiple of 128.
 *      Limits and codes are vcap_gpt2_score's, refused before any launch: B * S <= vcap_gpt2_max_rows(),
 *      S <= n_positions (VCAP_E_UNSUPPORTED); both decoder dtypes; a grad desc whose dtype / n_embd /
 *      n_layer differ from the decoder's or whose vocab_pad is not the padded vocabulary, null pointers and
 *      bad sizes: VCAP_E_ARG; a small workspace: VCAP_E_WORKSPACE (the query returns 0 outside the limits).
 *      Not graph-captured; leaves no KV state.
 *      Contracts:
 *        - logprob_out and loss_out are bit-identical to vcap_gpt2_score's: the forward is that schedule,
 *          with copies of the f32 residual stream (each layer's input, after each attention c_proj, the last
 *          layer's output) taken between its launches.
 *        - Deterministic: fixed reduction orders and no float atomics; two calls give the same bits.
 *        - Batch-independent: the bits of sequence b's gradient depend on its own embeds, mask, targets and
 *          weights, S and the model only - not on B nor on the other sequences.  Every product runs one
 *          128x128-tile kernel at every row count (vcap_set_gemm_policy is not followed); its K range is cut
 *          into slabs of a constant width (256 columns in the block products, 2048 in the K = vocab product
 *          of the lm_head), a function of the model's shape alone, summed in slab order.
 *        - Exact zeros: the gradient is exactly +0 at a position after its sequence's last counted
 *          position, everywhere in a sequence with no counted position, and at a hidden key whose own
 *          target is ignored.
 *      Rounding points with a bf16 decoder (an f32 decoder rounds nowhere): every MFMA operand is bf16 (RNE) -
 *      the recomputed LayerNorm rows, dlogit = w (onehot - softmax), the residual gradient where it enters
 *      the two c_proj^T products, du = dact * gelu_new'(u), dq | dk | dv - and the recomputed q | k | v are
 *      rounded to bf16 values as the forward stores them.  Accumulation, the residual gradient stream and
 *      the softmax / LayerNorm / GELU backward arithmetic are f32; the attention backward is f32 throughout. ---- */
typedef struct vcap_gpt2_grad_layer {
  const void* attn_c;        /* [E, 3E]  c_attn Conv1D as stored */
  const void* aproj_c;       /* [E, E]   attn c_proj */
  const void* fc_c;          /* [E, 4E]  mlp c_fc */
  const void* mproj_c;       /* [4E, E]  mlp c_proj */
  const void* attn_l;        /* [3E, E]  c_attn transposed (Linear layout) */
  const void* fc_l;          /* [4E, E]  c_fc transposed */
} vcap_gpt2_grad_layer;

typedef struct vcap_gpt2_grad_desc {
  int dtype, n_embd, n_layer;  /* the decoder's */
  int vocab_pad;               /* vocab rounded up to a multiple of 128 */
  const void* wte_t;           /* [E, vocab_pad]: wte transposed, columns >= vocab zero */
  const vcap_gpt2_grad_layer* layers;  /* host array of n_layer entries */
} vcap_gpt2_grad_desc;

size_t vcap_gpt2_score_backward_workspace_bytes(const vcap_gpt2_desc* d, const vcap_gpt2_grad_desc* g, int B, int S);
int vcap_gpt2_score_backward(const vcap_gpt2_desc* d, const vcap_gpt2_grad_desc* g, const float* embeds, int B, int S,
                             const uint8_t* key_mask, const int* targets, const float* grad_logprob,
                             float* grad_embeds, float* logprob_out, float* loss_out, void* workspace,
                             size_t ws_bytes, void* stream);

/* ---- GPT-2 tail fine-tuning (added within ABI v16: new symbols and two new structs, nothing existing
 *      changes): vcap_gpt2_score_backward plus the gradient of the same objective with respect to every
 *      parameter of the last n_tail blocks - the reference's --unfreeze_gpt2_last N
 *      (src/cli/train_caption_mapper.py: block.parameters() of transformer.h[-N:]; ln_f, wte and wpe stay
 *      frozen).  One walk serves both entry points: this call is that walk with side outputs, so
 *        - grad_embeds (required here too: the mapper trains as well), logprob_out and loss_out are
 *          bit-identical to vcap_gpt2_score_backward's on the same inputs.
 *      param_grads->layers[i] holds the 12 device f32 outputs of layer n_layer - n_tail + i in HF's own
 *      layouts (Conv1D weights [in, out]); they are written, not accumulated.  In an unfrozen layer the walk
 *      emits, from operands it holds at that point (T = the decoder dtype):
 *          d mproj_w = act^T . g    d mproj_b = colsum(g)       act = gelu_new(c_fc), the forward's own bits
 *          d fc_w    = xn2^T . du   d fc_b    = colsum(du)      xn2 = ln_2(x1) recomputed, du = dact gelu'(u)
 *          d ln2_g   = sum_m dy xhat(x1)   d ln2_b = sum_m dy   dy = du . c_fc^T (f32)
 *          d aproj_w = att^T . g'   d aproj_b = colsum(g')      att = the forward's attention output, g' = the
 *                                                              residual gradient after the ln_2 backward
 *          d attn_w  = xn1^T . dqkv d attn_b  = colsum(dqkv)    xn1 = ln_1(x0) recomputed
 *          d ln1_g, d ln1_b likewise from dy = dqkv . c_attn^T and x0
 *      g / g' enter as the T copy the c_proj^T products already read (bf16: RNE of the f32 stream).  act and
 *      att are two more copies per unfrozen layer taken between the forward's launches (M * 5E elements of T
 *      per layer); frozen layers cost nothing, and vcap_gpt2_score / vcap_gpt2_score_backward take none.
 *      Each product dW[k][n] = sum_m X[m][k] dY[m][n] is ONE launch (vcap_gpt2_dw_kernel,
 *      csrc/gpt2_weight_grad.hip): a workgroup owns a 64 x 128 tile of dW - a function of (K, N) alone - and
 *      sums all M <= 512 rows in ascending 32-row tiles, X and dY read row-major as they lie and consumed
 *      column-wise from LDS (bf16: ds_read_b64_tr_b16); rows past M are zero-filled.  No split of the row
 *      axis, no slabs, no atomics.  Column sums: wave w of a column's workgroup adds rows w, w + 4, ... and the
 *      four partials are added in wave order.  Accumulation is f32 everywhere; with a bf16 decoder the
 *      products' operands are bf16 (the call's existing rounding points) and nothing else rounds.
 *      Contracts beside vcap_gpt2_score_backward's:
 *        - Deterministic: two calls give the same bits.
 *        - Linear in grad_logprob: doubling it doubles every parameter gradient bit for bit.
 *        - Exactly +0 everywhere when no position is counted.
 *        - Appending sequences with no counted position leaves every parameter gradient bit-identical (their
 *          dY rows are zeros and no reduction order depends on M).
 *      Refused before any launch, outputs untouched: vcap_gpt2_score_backward's refusals with its codes;
 *      n_tail outside 1 .. n_layer, a null struct or any null gradient pointer: VCAP_E_ARG; a small workspace:
 *      VCAP_E_WORKSPACE (the query returns 0 outside the limits). ---- */
typedef struct vcap_gpt2_param_grads_layer {   /* device f32, HF's layouts */
  float *ln1_g, *ln1_b, *attn_w /* [E, 3E] */, *attn_b, *aproj_w /* [E, E] */, *aproj_b;
  float *ln2_g, *ln2_b, *fc_w /* [E, 4E] */, *fc_b, *mproj_w /* [4E, E] */, *mproj_b;
} vcap_gpt2_param_grads_layer;

typedef struct vcap_gpt2_param_grads {
  int n_tail;                                  /* 1 .. n_layer */
  const vcap_gpt2_param_grads_layer* layers;   /* host array; entry i = layer n_layer - n_tail + i */
} vcap_gpt2_param_grads;

size_t vcap_gpt2_score_backward_tail_workspace_bytes(const vcap_gpt2_desc* d, const vcap_gpt2_grad_desc* g, int B,
                                                     int S, int n_tail);
int vcap_gpt2_score_backward_tail(const vcap_gpt2_desc* d, const vcap_gpt2_grad_desc* g, const float* embeds, int B,
                                  int S, const uint8_t* key_mask, const int* targets, const float* grad_logprob,
                                  float* grad_embeds, const vcap_gpt2_param_grads* param_grads, float* logprob_out,
                                  float* loss_out, void* workspace, size_t ws_bytes, void* stream);
/* The tail call's product alone (kernel tests and measurements): dW [K, N] f32 = X^T . dY over the M rows of
 * X [M, K] and dY [M, N], both row-major device memory in `dtype` (VCAP_DT_F32 or VCAP_DT_BF16), 16-byte
 * aligned.  Rows at and past M are never read.  VCAP_E_ARG: dtype, null / unaligned pointers, sizes < 1;
 * VCAP_E_UNSUPPORTED: M > vcap_gpt2_max_rows(), K % 64 != 0 or N % 128 != 0. */
int vcap_gpt2_weight_grad(int dtype, const void* X, const void* dY, float* dW, int M, int K, int N, void* stream);

/* ---- video retrieval (added within ABI v16: new symbols only, no struct changes): the inference half of
 *      the reference's second product - embed a clip, search a flat inner-product index of clip
 *      embeddings.  Reference interfaces: ViTTextAlignModel.encode_video
 *      (src/models/vit_text_align.py:54-65) = ViTFrameEncoder(pool="cls", l2norm=True)
 *      (src/models/video_encoder.py:318-319), i.e. vcap_vit_encode's enc_out followed by
 *      vcap_l2_normalize; faiss.normalize_L2 + faiss.IndexFlatIP.add (scripts/build_index.py:40-42);
 *      the l2norm helper, index.search and the printed neighbours of scripts/query_video.py:20-21,
 *      61-75, 127.  All pointers are device memory; nothing allocates or synchronises; no graph is
 *      captured, and every call is safe inside a caller's capture.
 *
 *      vcap_l2_normalize: rows of f32 [rows, dim] (row strides ldx / ldy, y == x allowed).
 *        eps_mode 0: y = x / max(||x||, eps)   F.normalize (eps 1e-12); a zero row stays zero, as under
 *                                              faiss.normalize_L2
 *        eps_mode 1: y = x / (||x|| + eps)     query_video.py / eval_retrieval.py l2norm (eps 1e-8)
 *        The sum of squares is an f32 fma chain per lane (elements l, l + 64, ...) and a fixed tree over
 *        the 64 lanes: a row's result does not depend on `rows`.
 *      vcap_ip_index_convert: f32 rows [rows, dim] (row stride ldx) -> contiguous index storage
 *        [rows, dim]: VCAP_DT_F32 a copy, VCAP_DT_BF16 round-to-nearest-even with NaN -> 0x7FC0,
 *        bit-identical to torch.Tensor.to(torch.bfloat16).  dim % 4 == 0, ldx % 4 == 0, 16-byte aligned
 *        pointers (VCAP_E_UNSUPPORTED otherwise).
 *      vcap_ip_search: exact top-k by inner product.  db [n, dim] contiguous, VCAP_DT_F32 or
 *        VCAP_DT_BF16 (widened to f32, exact); queries [nq, dim] f32; out_scores [nq, k] f32 and out_ids
 *        [nq, k] int64; max_blocks as vcap_gen_params.max_blocks (0: whole chip).
 *        Limits (VCAP_E_UNSUPPORTED before any launch): dim % 64 == 0 and 64 <= dim <= 1024;
 *        1 <= k <= 128; 1 <= nq <= 64 and nq * dim <= 16384; 0 <= n < 2^31 rows (n * dim may pass 2^31:
 *        offsets are 64-bit); db and queries 16-byte aligned.  Null pointers, negative sizes and other
 *        dtypes: VCAP_E_ARG.
 *        Contract: the f32 score of row i against query q is one fixed-order f32 fma chain over the
 *        row's elements - a function of (row, query, dim, storage dtype) only, not of i, n, nq, the
 *        query's slot, the grid, max_blocks or a CU mask.  |score - exact| <= 2 * dim * 2^-24 * ||q|| ||x||.
 *        Results are ordered by score descending, then id ascending (+0 and -0 compare equal), so the
 *        output is unique: any two calls, grids or batchings of the same rows give the same bits.
 *        A row whose score is NaN is never returned.  Where fewer than k rows remain (k > n, NaN
 *        rows) the tail is id -1 with score -inf (our filler; FAISS's own was not available to compare).
 *        The database is read once per pass of up to 16 * max(1, min(4, 1024 / dim)) queries (one pass
 *        for nq <= 16 at every dim, for nq <= 64 up to dim 256); dot products run on the f32-input MFMA.
 *      vcap_ip_search_workspace_bytes: the caller-owned workspace (0 outside the limits): per scan
 *        workgroup and query k + 2 * vcap_ip_search_slab_rows() 8-byte candidate slots, for
 *        min(512, ceil(n / slab rows)) workgroups.
 *      vcap_ip_search_slab_rows / vcap_ip_search_workgroups: the rows a scan workgroup takes per step
 *        and the scan grid for n rows under max_blocks on the current device (workgroup w takes slabs
 *        w, w + grid, ...) - for tests that place rows on slab and workgroup boundaries. ---- */
int vcap_l2_normalize(const float* x, int64_t ldx, float* y, int64_t ldy, int rows, int dim, float eps, int eps_mode,
                      void* stream);
int vcap_ip_index_convert(const float* x, int64_t ldx, int rows, int dim, int storage_dtype, void* dst, void* stream);
size_t vcap_ip_search_workspace_bytes(int64_t n, int dim, int nq, int k);
int vcap_ip_search(int storage_dtype, const void* db, int64_t n, int dim, const float* queries, int nq, int k,
                   float* out_scores, int64_t* out_ids, void* workspace, size_t ws_bytes, int max_blocks,
                   void* stream);
int vcap_ip_search_slab_rows(void);
int vcap_ip_search_workgroups(int64_t n, int max_blocks);

/* ---- IVF-Flat inner-product index (added within ABI v16: new symbols only): the reference's
 *      faiss.IndexIVFFlat(IndexFlatIP(d), d, nlist, METRIC_INNER_PRODUCT) of
 *      scripts/build_index_with_captions.py (--index_type IVF_FLAT --nlist 50): a coarse quantiser over
 *      nlist centroids, the stored rows grouped into nlist inverted lists, and a search that scans the
 *      nprobe lists whose centroids score best.  As for the flat search: device pointers only, nothing
 *      allocates or synchronises, no float atomics, no spinning, safe inside a caller's capture.
 *      Common limits (VCAP_E_UNSUPPORTED before any launch): dim % 64 == 0 and 64 <= dim <= 1024;
 *      1 <= nlist <= 1048576; row counts below 2^31; f32 rows and centroids 16-byte aligned with row
 *      strides in whole 16-byte vectors.  Null pointers and negative sizes: VCAP_E_ARG.
 *
 *      vcap_ivf_assign: rows f32 [n, dim] (row stride ldx), centroids f32 [nlist, dim] contiguous ->
 *        assign int32 [n] and, where score is not null, score f32 [n].  One launch reads the rows once: a
 *        workgroup stages up to 64 rows and walks the centroid tiles on the f32-input MFMA with a running
 *        arg-max per row.
 *        Contract: the score of (row, centroid) has the bits vcap_ip_search(db = centroids, queries = row)
 *        returns (the same fma chain over the same element permutation, the same operand roles).  The
 *        winner is the largest score, the lowest centroid id on equal scores (+0 and -0 compare equal);
 *        a NaN score never wins; a row whose scores are all NaN gets assign -1 and score -inf.  So
 *        assign / score equal the k = 1 output of vcap_ip_search over the centroids, and a stored f32
 *        vector used as a query probes its own list first.
 *      vcap_ivf_centroid_update: one spherical k-means update.  order int64 [n]: row indices grouped by
 *        list, ascending within a list; offsets int64 [nlist + 1]: list l owns order[offsets[l],
 *        offsets[l + 1]) (offsets[0] may exceed 0: leading entries of order belong to no list).
 *        out [nlist, dim] (out == prev allowed) = the f32 sum of the list's member rows, L2-normalised with
 *        vcap_l2_normalize's mode-0 arithmetic (eps 1e-12).  On unit rows, arg-max inner product against
 *        unit centroids is the arg-min L2 assignment FAISS trains with.  An empty list keeps its previous
 *        centroid (FAISS splits a large cluster instead; this library does not).
 *        Order of summation: members [c * R, (c + 1) * R) of a list (R = vcap_ivf_chunk_rows() = 512) are
 *        added in order by one wave starting from 0, and the chunks' partial sums are added in chunk order
 *        by a second kernel.  A centroid's bits depend on its member rows in `order` order only - not on
 *        the other lists, the grid or a CU mask.  An index in order outside [0, n) is skipped.
 *        Workspace (16-byte aligned): vcap_ivf_centroid_update_workspace_bytes(n, nlist, dim) =
 *        (n / R + nlist + 1) rows of dim f32, rounded up to 256 bytes; 0 outside the limits.
 *      vcap_ivf_search: rows [ntotal, dim] VCAP_DT_F32 or VCAP_DT_BF16, grouped by list; ids int64
 *        [ntotal] (each row's original id, unique, 0 <= id < 2^31); offsets int64 [nlist + 1] with
 *        offsets[0] = 0 and offsets[nlist] = ntotal; max_list_len: the host's copy of the longest list's
 *        length (it sizes the scan grid; rows of a list beyond it are not scanned); out_probes optional
 *        int64 [nq, nprobe].  Three stages on `stream`:
 *          (a) coarse: vcap_ip_search's own dispatch over the centroids with k = nprobe -> the probed
 *              list ids on the device (also into out_probes), best first, -1 where fewer than nprobe
 *              centroids have a non-NaN score;
 *          (b) list scan: one workgroup per (query, probe, slice of vcap_ivf_slice_rows() = 512 rows of
 *              the list), grid ceil(max_list_len / 512) x nprobe x nq; items past their list's end leave
 *              empty slots.  Each row is scored with the flat scan's chain, so the bits equal
 *              vcap_ip_search's score of that (row, query, storage dtype); an item keeps its best k keys
 *              (score, original id) in the workspace.  List starts are not padded: a tile's rows past the
 *              slice's end read the slice's last row and are dropped, as in the flat scan;
 *          (c) merge: vcap_ip_search's merge kernel over the items' lists, one workgroup per query.
 *        Contract: the output is the exact top-k, score descending then id ascending, over the union of
 *        the rows of the probed lists; id -1 / score -inf where fewer than k exist; a row whose score is
 *        NaN is never returned.  The output is unique: two calls, grids, max_blocks (it bounds the coarse
 *        scan's grid only), CU masks or query batchings give the same bits, and with nprobe == nlist (no
 *        NaN centroid) it is bit-identical to vcap_ip_search over the same vectors with the same ids.
 *        Limits beyond the common ones: 1 <= k <= 128; 1 <= nprobe <= 128 (nprobe > nlist only adds -1
 *        probes; callers clamp); 1 <= nq <= 64 and nq * dim <= 16384; max_list_len <= ntotal < 2^31
 *        (VCAP_E_ARG when it exceeds ntotal); a storage dtype other than F32 / BF16: VCAP_E_ARG; a short
 *        workspace: VCAP_E_WORKSPACE.  The kernel reads no list whose offsets fall outside [0, ntotal].
 *      vcap_ivf_search_workspace_bytes: the coarse search's workspace (vcap_ip_search_workspace_bytes(nlist,
 *        dim, nq, nprobe)) + the probes and their scores + ceil(max_list_len / 512) * nprobe * nq * k
 *        8-byte key slots, each piece rounded up to 256 bytes; 0 outside the limits.
 *        Cost: the scan grid, the key workspace and the merge (one workgroup per query walking
 *        ceil(max_list_len / 512) * nprobe * k slots) all scale with the LONGEST list, not with the lists a
 *        query probes: with skewed lists most items only write k empty slots and the merge reads them. ---- */
int vcap_ivf_slice_rows(void);
int vcap_ivf_chunk_rows(void);
int vcap_ivf_assign(const float* x, int64_t ldx, int64_t n, const float* centroids, int nlist, int dim, int32_t* assign,
                    float* score, void* stream);
size_t vcap_ivf_centroid_update_workspace_bytes(int64_t n, int nlist, int dim);
int vcap_ivf_centroid_update(const float* x, int64_t ldx, int64_t n, int dim, const int64_t* order,
                             const int64_t* offsets, int nlist, const float* prev, float* out, void* workspace,
                             size_t ws_bytes, void* stream);
size_t vcap_ivf_search_workspace_bytes(int nlist, int64_t max_list_len, int dim, int nq, int nprobe, int k);
int vcap_ivf_search(int storage_dtype, const void* rows, const int64_t* ids, const int64_t* offsets, int64_t ntotal,
                    const float* centroids, int nlist, int64_t max_list_len, int dim, const float* queries, int nq,
                    int nprobe, int k, float* out_scores, int64_t* out_ids, int64_t* out_probes, void* workspace,
                    size_t ws_bytes, int max_blocks, void* stream);

/* ---- text tower (added within ABI v16: new symbols and structs only): ViTTextAlignModel.encode_text
 *      (src/models/vit_text_align.py:67-79) - nn.Embedding -> nn.TransformerEncoder of post-LN ReLU
 *      nn.TransformerEncoderLayer(batch_first) -> mean over the positions whose id != pad_id (count
 *      clamped to >= 1) -> txt_proj -> F.normalize (eps 1e-12).  As in the reference, the encoder gets no
 *      key-padding mask: pad positions are ordinary keys and queries and only the pool leaves them out; the
 *      pad row of the table is gathered as stored; an all-pad caption comes out as normalize(proj_b).
 *        ids         device [B][L]; an id outside [0, vocab) reads nothing and makes that caption's
 *                    embedding (and its hidden_out rows) NaN, no other caption's
 *        out         device [B][proj_dim] f32, unit rows
 *        hidden_out  optional device [B][L][dim] f32: the encoder output before the pool
 *      Limits (refused before any launch): dim % 128 == 0, dim <= 1024, n_head * 64 == dim; ffn % 128 == 0,
 *      ffn <= 4096; proj_dim % 64 == 0, 64 <= proj_dim <= 1024; 1 <= L <= 64, B * L <= vcap_gpt2_max_rows();
 *      emb, proj_w and the workspace 16-byte aligned (VCAP_E_UNSUPPORTED).  Null pointers, a dtype other
 *      than VCAP_DT_F32 / VCAP_DT_BF16, a pad_id outside [0, vocab), n_layer < 0 and B < 1: VCAP_E_ARG.
 *      A short workspace: VCAP_E_WORKSPACE.
 *      About 2 + 7 * n_layer launches on `stream`; deterministic (fixed reduction orders, no float
 *      atomics: two calls on the same inputs give the same bits, with or without hidden_out); not
 *      graph-captured; leaves no state.  vcap_text_workspace_bytes returns 0 outside the limits. ---- */
typedef struct vcap_text_layer {      /* projection weights rows-packed by vcap_rows_pack, biases / LN f32 */
  const void* in_w;  const float* in_b;   /* [3E, E] self_attn.in_proj_*   */
  const void* out_w; const float* out_b;  /* [E, E]  self_attn.out_proj.*  */
  const float* ln1_g; const float* ln1_b;
  const void* fc1_w; const float* fc1_b;  /* [F, E]  linear1 */
  const void* fc2_w; const float* fc2_b;  /* [E, F]  linear2 */
  const float* ln2_g; const float* ln2_b;
} vcap_text_layer;
typedef struct vcap_text_desc {
  int dtype;                  /* VCAP_DT_F32 | VCAP_DT_BF16: GEMV operands, q/k/v, activations.  Residual stream,
                                 LayerNorm, softmax, pool, projection and normalisation are f32 in both. */
  int vocab, dim, n_layer, n_head, ffn, proj_dim, pad_id;
  float ln_eps;               /* 1e-5 */
  const float* emb;           /* [vocab, dim] f32 */
  const float* proj_w; const float* proj_b;   /* [proj_dim, dim], [proj_dim] f32 */
  const vcap_text_layer* layers;              /* host array of n_layer entries; may be NULL when n_layer == 0 */
} vcap_text_desc;
size_t vcap_text_workspace_bytes(const vcap_text_desc* d, int B, int L);
int vcap_text_encode(const vcap_text_desc* d, const int* ids /* device [B][L] */, int B, int L,
                     float* out /* device [B][proj_dim], unit rows */,
                     float* hidden_out /* optional device [B][L][dim]: the encoder output before the pool */,
                     void* workspace, size_t ws_bytes, void* stream);

/* ---- text tower training (added within ABI v16: new symbols and structs only): the gradient of any scalar of
 *      vcap_text_encode's unit-norm `out` rows with respect to every text-tower parameter - autograd of
 *      ViTTextAlignModel.encode_text in eval mode (no dropout).  One call runs vcap_text_encode's schedule,
 *      keeping per layer the f32 stream at the layer input, the two pre-LayerNorm sums, the LN1 output, q | k | v,
 *      the attention output and the ReLU output, then walks the layers last to first.  `out` has
 *      vcap_text_encode's bits.
 *        grad_out    device [B][proj_dim] f32: d scalar / d out
 *        grads       device f32 tensors in torch's own layouts ([out, in]); every pointer required
 *        emb_ids / emb_rows / emb_count   the row-sparse embedding gradient: emb_ids[0 .. count) = the distinct
 *                    ids of the call that are neither pad_id nor outside the vocabulary, ascending; emb_rows[i] =
 *                    the f32 sum of the layer-0 input gradient over the positions holding emb_ids[i], in
 *                    ascending flat position b * L + l, from +0; entries count .. B*L-1 are id -1 with zero rows
 *      The grad desc holds operand-dtype, plain row-major TRANSPOSED ([in, out]) copies of the four
 *      projection weights of each layer: every dx = dy . W is then C = A . Wt^T on the 128x128 MFMA tile
 *      kernel.  Weight gradients dW = dY^T . X run on the same kernel over operand-dtype transposed copies
 *      dY^T [N][Mpad], X^T [K][Mpad] (Mpad = B*L rounded up to the K tile, 32 rows f32 / 64 bf16, the pad
 *      columns +0).  No float atomics; every sum over the B*L rows has one order that depends on the model
 *      shape and (B, L) only: K tiles in order inside constant slabs of 128 rows added in slab order (weights);
 *      rows w, w + 4, ... per wave w = 0..3, the four partial sums added in wave order (biases, gamma / beta);
 *      captions in order (proj_w, proj_b).  A caption with no non-pad position contributes exactly +0 to
 *      everything upstream of the pool.  An id outside [0, vocab) is never used as an index; it makes the
 *      call's weight gradients NaN.  bf16: every MFMA operand is bf16 (RNE); accumulation, the residual gradient,
 *      the attention, LayerNorm and tail arithmetic are f32; an f32 desc rounds nowhere.
 *      Limits and return codes are vcap_text_encode's, refused before the first launch; a grad desc whose
 *      dtype / dim / ffn / n_layer differ from the text desc's and null gradient or weight pointers are
 *      VCAP_E_ARG, a short workspace VCAP_E_WORKSPACE; the workspace query returns 0 outside the limits.
 *      n_layer == 0 works (embedding -> pool -> proj).  6 + 46 * n_layer launches and device copies (50 * n_layer
 *      with bf16 operands: the row gradients' bf16 copies). ---- */
typedef struct vcap_text_grad_layer {     /* operand dtype, row-major [in, out] */
  const void* in_t;    /* [E, 3E] = in_proj_weight^T  */
  const void* out_t;   /* [E, E]  = out_proj.weight^T */
  const void* fc1_t;   /* [E, F]  = linear1.weight^T  */
  const void* fc2_t;   /* [F, E]  = linear2.weight^T  */
} vcap_text_grad_layer;
typedef struct vcap_text_grad_desc {
  int dtype, dim, ffn, n_layer;           /* must equal the text desc's */
  const vcap_text_grad_layer* layers;     /* host array of n_layer entries; may be NULL when n_layer == 0 */
} vcap_text_grad_desc;
typedef struct vcap_text_param_grads_layer {   /* device f32 */
  float* in_w;  float* in_b;    /* [3E, E], [3E] */
  float* out_w; float* out_b;   /* [E, E], [E]   */
  float* ln1_g; float* ln1_b;
  float* fc1_w; float* fc1_b;   /* [F, E], [F]   */
  float* fc2_w; float* fc2_b;   /* [E, F], [E]   */
  float* ln2_g; float* ln2_b;
} vcap_text_param_grads_layer;
typedef struct vcap_text_param_grads {
  float* proj_w; float* proj_b;           /* [proj_dim, dim], [proj_dim] */
  int* emb_ids; float* emb_rows;          /* [B*L], [B*L][dim] */
  int* emb_count;                         /* device scalar */
  const vcap_text_param_grads_layer* layers;   /* host array of n_layer entries */
} vcap_text_param_grads;
size_t vcap_text_encode_backward_workspace_bytes(const vcap_text_desc* d, const vcap_text_grad_desc* g, int B, int L);
int vcap_text_encode_backward(const vcap_text_desc* d, const vcap_text_grad_desc* g, const int* ids /* device */,
                              int B, int L, const float* grad_out, const vcap_text_param_grads* grads,
                              float* out /* device [B][proj_dim] */, void* workspace, size_t ws_bytes, void* stream);

/* ---- ragged prompts (added within ABI v16: new symbols and one struct only): one device decode for B
 *      rows with a prompt each.  The contract is per row: row b's tokens, raw logits, warped scores and
 *      beam result are those of the uniform entry point (vcap_gpt2_generate / _sample / _beam_search)
 *      called with B = 1, prefix row b and prompt b.  Output layouts are the uniform calls':
 *      out_ids [B][max_new], logits_out / warped_out [max_new][B][vocab], force_ids [B][max_new],
 *      beam out_ids [B][max_new] + out_len [B].  A sampling row b draws from Philox counter (step, b), so
 *      only row 0's free draw is the B = 1 call's draw; with force_ids every row's warped scores are.
 *      The prefill packs its rows with no padding, sequence-major: M = sum_b (prefix_len + len_b) rows
 *      (times num_beams for the search's replicated prefill).  Sequence b occupies positions
 *      0 .. S0_b - 1 (S0_b = prefix_len + len_b) and its step t runs at position S0_b + t.  The
 *      processors see generated tokens only.  The prompt ids and the row tables are uploaded to the
 *      workspace on `stream` before the first launch, outside the captured graph: one graph (keyed by B,
 *      the offsets, the parameters and the pointers) serves every set of ids with those lengths.
 *      Limits, each refused before any launch (the workspace queries return 0): every len_b in [0, 64]
 *      and S0_b > 0; M <= vcap_gpt2_max_rows(); S0_b + max_new <= n_positions; offsets[0] == 0 and
 *      non-decreasing; ids inside the vocabulary; beam search also B <= 8, 2 <= num_beams <= 8,
 *      max_new <= 64 and max_b S0_b + max_new <= 128.  VCAP_E_ARG / VCAP_E_UNSUPPORTED as the uniform
 *      calls give them. ---- */
typedef struct vcap_prompts {   /* host memory */
  const int* ids;       /* the B prompts concatenated (may be NULL when every prompt is empty) */
  const int* offsets;   /* [B + 1], offsets[0] == 0, non-decreasing; prompt b = ids[offsets[b] .. offsets[b+1]) */
} vcap_prompts;
size_t vcap_gpt2_ragged_workspace_bytes(const vcap_gpt2_desc* d, const int* offsets, int B, int max_new_tokens);
int vcap_gpt2_generate_ragged(const vcap_gpt2_desc* d, const vcap_gen_params* gp, const float* prefix,
                              const vcap_prompts* prompts, int B, int* out_ids, float* logits_out, void* workspace,
                              size_t ws_bytes, void* stream);
int vcap_gpt2_sample_ragged(const vcap_gpt2_desc* d, const vcap_gen_params* gp, const vcap_sample_params* sp,
                            const float* prefix, const vcap_prompts* prompts, int B, int* out_ids, float* logits_out,
                            float* warped_out, const int* force_ids, void* workspace, size_t ws_bytes, void* stream);
size_t vcap_gpt2_beam_search_ragged_workspace_bytes(const vcap_gpt2_desc* d, const int* offsets, int B, int num_beams,
                                                    int max_new_tokens);
int vcap_gpt2_beam_search_ragged(const vcap_gpt2_desc* d, const vcap_beam_params* bp, const float* prefix,
                                 const vcap_prompts* prompts, int B, int* out_ids, int* out_len, void* workspace,
                                 size_t ws_bytes, void* stream);

/* ---- ViT training (added within ABI v16: new symbols and structs only): the gradient of any scalar of
 *      vcap_vit_encode's enc_out with respect to the encoder's trainable parameters - autograd of
 *      ViTFrameEncoder.forward as src/cli/train_full.py --model vit trains it (timm's ViT has no dropout).
 *      One call runs vcap_vit_encode's schedule and walks back through the last n_tail blocks (1 .. depth).
 *      It returns, as device f32 tensors in timm's own layouts, the gradients of encoder.proj (weight, bias),
 *      the final norm (gamma, beta) and the 12 tensors of each of the last n_tail blocks; with n_tail == depth
 *      also patch_embed.proj.weight (as [dim, kpad]: the flattened [dim, 3*p*p] kernel, pad columns +0),
 *      patch_embed.proj.bias, cls_token [dim] and pos_embed [tokens, dim]; those four pointers may be NULL
 *      otherwise.  grads->layers[j] is block depth - n_tail + j.  Blocks below the tail run exactly as
 *      vcap_vit_encode runs them and keep nothing; the walk stops at the first unfrozen block's input.
 *      enc_out has vcap_vit_encode's bits: in the unfrozen blocks the QKV projection + attention run as the
 *      GEMM + attention pair (bit-identical to the fused kernel), the last block stays the CLS-only tail.
 *      Per unfrozen block the forward keeps the f32 stream at the block input and after the attention
 *      residual, q | k | v, the attention output and the GELU output (operand dtype); the LayerNorm outputs and
 *      the fc1 pre-activation are recomputed, the latter in f32 (fc1 without its GELU epilogue), so gelu' is
 *      never taken from a rounded pre-activation.
 *      The grad desc holds operand-dtype, plain row-major TRANSPOSED ([in, out]) copies of the four Linear
 *      weights of every block (blocks below the tail are not read and may be NULL) and, for the caller's
 *      bookkeeping only, the f32 masters they were rounded from (never dereferenced by the library).
 *      Operand dtypes: VCAP_DT_F32 and VCAP_DT_BF16; VCAP_DT_F16 and VCAP_DT_MXFP8 are VCAP_E_UNSUPPORTED
 *      before any launch.  Widths: dim % 128 == 0 (head dim 64, dim <= 1024: ViT-S / B / L) and mlp % 128 == 0
 *      are served, every other width is VCAP_E_UNSUPPORTED before any launch; token counts are the ones
 *      vcap_vit_encode serves in these dtypes (1..32, 193..224, 257..288).
 *      bf16: every MFMA operand is bf16 (RNE) - q | k | v, P, dS, dO and each Linear's dY once, when it enters a
 *      product; accumulation, the residual gradient, softmax, LayerNorm / GELU backward and all bias / affine
 *      sums are f32.  An f32 desc rounds nowhere.  No float atomics; every sum has one order that depends on
 *      (B, T, n_tail, the architecture) only: 32-row tiles in order inside constant 256-row slabs added in slab
 *      order (weights); rows w, w + 4, ... per wave w = 0..3, partials added in wave order (biases, gamma,
 *      beta); frames in order (pos, cls); videos in order (encoder.proj).  A video whose grad_out row is +0
 *      adds exactly +0 to every gradient; doubling grad_out doubles every gradient exactly.
 *      Alignment: the workspace 256-byte aligned; the grad desc's transposed copies (qkv_t, proj_t, fc1_t, fc2_t
 *      of the unfrozen blocks) and the weight gradients (qkv_w, proj_w, fc1_w, fc2_w of every returned block,
 *      patch_w) 16-byte aligned; frames, grad_out and the other gradients need their element alignment only.
 *      Size of one call: B * T * heads <= 65535 and B * T * tokens <= 2^22 (larger batches go in chunks, whose
 *      gradients the caller adds).
 *      Return codes, every one before the first launch and writing nothing (the workspace query returns 0
 *      outside the limits): VCAP_E_ARG - null pointers (a NULL embedding gradient only with n_tail == depth),
 *      B / T < 1, n_tail outside 1 .. depth, a grad desc whose dtype / dim / mlp / depth differ from the vit
 *      desc's; VCAP_E_UNSUPPORTED - the descriptor limits of vcap_vit_encode, an operand dtype or width outside
 *      the ones above, a call over the size limits, a workspace that is not 256-byte aligned, a transposed copy or
 *      weight gradient that is not 16-byte aligned; VCAP_E_WORKSPACE - ws_bytes below
 *      vcap_vit_backward_workspace_bytes.
 *      One training step through an autograd wrapper that calls vcap_vit_encode in its forward and this call in
 *      its backward (vcap.train_align.EncodeVideo) runs the encoder forward twice: once for enc_out, once more
 *      inside this call, which keeps no state between calls.
 *      vcap_vit_attention_backward is the attention backward alone, at every token count 1..288: qkv
 *      [frames*tokens][3*64*heads] in `dtype`, dout f32 [frames*tokens][64*heads] -> dqkv f32 (dq | dk | dv).
 *      Per (frame, head): S = Q K^T / 8 and the softmax by the forward kernels' expressions, dP = dO V^T,
 *      delta = rowsum(P dP), dS = P (dP - delta) / 8, dQ = dS K, dK = dS^T Q, dV = P^T dO on the MFMA; keys
 *      past the token count contribute exactly 0.  Null pointers and sizes < 1: VCAP_E_ARG; another dtype,
 *      tokens > 288, frames * heads > 65535, qkv / dout / dqkv not 16-byte or the workspace not 256-byte aligned:
 *      VCAP_E_UNSUPPORTED (the workspace query returns 0), all before any launch. ---- */
typedef struct vcap_vit_grad_layer {
  const void* qkv_t;   /* [D, 3D]  = attn.qkv.weight^T,  operand dtype */
  const void* proj_t;  /* [D, D]   = attn.proj.weight^T */
  const void* fc1_t;   /* [D, mlp] = mlp.fc1.weight^T   */
  const void* fc2_t;   /* [mlp, D] = mlp.fc2.weight^T   */
  const float* qkv_m; const float* proj_m; const float* fc1_m; const float* fc2_m;   /* f32 masters, [out, in] */
} vcap_vit_grad_layer;
typedef struct vcap_vit_grad_desc {
  int dtype, dim, mlp, depth;              /* must equal the vit desc's */
  const vcap_vit_grad_layer* layers;       /* host array of depth entries */
} vcap_vit_grad_desc;
typedef struct vcap_vit_param_grads_layer {   /* device f32 */
  float* ln1_g; float* ln1_b;
  float* qkv_w; float* qkv_b;     /* [3D, D], [3D] */
  float* proj_w; float* proj_b;   /* [D, D], [D]   */
  float* ln2_g; float* ln2_b;
  float* fc1_w; float* fc1_b;     /* [mlp, D], [mlp] */
  float* fc2_w; float* fc2_b;     /* [D, mlp], [D]   */
} vcap_vit_param_grads_layer;
typedef struct vcap_vit_param_grads {
  float* proj_w; float* proj_b;   /* encoder.proj [video_dim, dim], [video_dim] */
  float* norm_g; float* norm_b;   /* [dim] */
  float* patch_w; float* patch_b; /* [dim, kpad], [dim]      (n_tail == depth) */
  float* cls; float* pos;         /* [dim], [tokens, dim]    (n_tail == depth) */
  const vcap_vit_param_grads_layer* layers;   /* host array of n_tail entries: blocks depth - n_tail .. depth - 1 */
} vcap_vit_param_grads;
size_t vcap_vit_backward_workspace_bytes(const vcap_vit_desc* d, int B, int T, int n_tail);
int vcap_vit_encode_backward(const vcap_vit_desc* d, const vcap_vit_grad_desc* g, const float* frames, int B, int T,
                             int n_tail, const float* grad_out /* device [B][video_dim] */,
                             float* enc_out /* device [B][video_dim] */, const vcap_vit_param_grads* grads,
                             void* workspace, size_t ws_bytes, void* stream);
size_t vcap_vit_attention_backward_workspace_bytes(int dtype, int frames, int tokens, int heads);
int vcap_vit_attention_backward(int dtype, const void* qkv, const float* dout, float* dqkv, int frames, int tokens,
                                int heads, void* workspace /* 256-byte aligned */, void* stream);

/* ---- live kernel timing for the benchmark's roofline (sites: "vit.qkv", "vit.attention",
 *      "vit.proj", "vit.fc1", "vit.fc2"): events are recorded around each launch of the site on
 *      the caller's stream, without synchronising; vcap_probe_read waits for them. ---- */
int vcap_probe_enable(const char* site, int max_launches);
int vcap_probe_read(const char* site, float* total_ms, int* launches);
/* Per-launch form: ms[i] / rows[i] (the launch's GEMM or attention rows) for each of the *launches
 * (<= cap) recorded launches; like vcap_probe_read it disables the site. */
int vcap_probe_read_launches(const char* site, float* ms, int* rows, int cap, int* launches);

#ifdef __cplusplus
}
#endif
#endif /* VCAP_H_ */
