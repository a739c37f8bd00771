// Kernel-side interface shared by the .hip translation units and the host runtime.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <string>

struct GemmEpi {
  const float* bias;  // [N] or nullptr
  const float* res;   // residual source (f32) or nullptr
  long ldr;           // residual row stride (elements)
  int act;            // 0 none, 1 gelu_tanh
  int res_mode;       // 0 none, 1 residual row == output row (may alias C), 2 row (m % G) + roff
  int G, Gs, goff;    // output row remap: G ? (m/G)*Gs + goff + m%G : m
  int roff;
  // MXFP8 operands (in_dt == VCAP_DT_MXFP8): E8M0 block scales of A and W, K-tile-major
  // (vcap_common.h); c_scale receives the scales of an MXFP8 output (act must be gelu).
  const uint8_t* a_scale;
  const uint8_t* w_scale;
  uint8_t* c_scale;
  // deterministic split-K (few-tile in-place residual GEMMs, bf16 operands): f32 partial slabs
  // [split][M][N]; the partials are summed in split order by a second kernel.  nullptr: no split.
  float* splitk_ws;
  size_t splitk_bytes;
  // 256x256 kernel tile order (set by its dispatcher): 0 = row-major over (row panel, column tile);
  // w > 0 = column groups of w tile columns, row-major inside a group
  int colgroup;
};

enum { PRO_LN = 0, PRO_DIRECT = 1 };
// EPI_LSE: raw logits -> logits_raw + per-workgroup (max, sum exp(x - max)) partials per row
// (part_val / part_sum): the log_softmax statistics of beam search
// EPI_STORE / EPI_RELU: T [M, ldo] = acc + bias / max(acc + bias, 0) (the text tower's in_proj and linear1)
// EPI_QKV_ROWS: EPI_QKV with row m's (sequence, position) read from the row tables (ragged prompts):
// seq = row_seq ? row_seq[m] : m, pos = row_pos[m] + pos_add; contiguous pages only
enum { EPI_QKV = 0, EPI_RESID = 1, EPI_GELU = 2, EPI_LOGITS = 3, EPI_STORE = 4, EPI_LSE = 5, EPI_RELU = 6,
       EPI_QKV_ROWS = 7 };

struct RowsGemmArgs {
  const void* x;  // PRO_LN: f32 residual rows; PRO_DIRECT: T rows
  long ldx;
  const float* ln_g;
  const float* ln_b;
  float ln_eps;
  const void* w;  // rows-packed T weights of a [N, K] matrix (vcap_rows_pack_dispatch)
  const float* bias;
  int M, N, K;
  void* out;  // RESID: f32 [M, ldo] (+=); GELU/STORE/RELU: T [M, ldo]
  long ldo;
  // QKV scatter into the paged cache
  void* q_out;            // T [M, E]
  void* kc;               // T pool: [pages][H][16][64] for this layer
  void* vc;
  const int* page_table;  // [seq][maxp]
  int maxp, H, S_new, past;
  // logits: processors + per-workgroup argmax partials
  float* logits_raw;  // optional [M, N] raw logits
  float* part_val;
  int* part_idx;
  float* part_sum;  // EPI_LSE
  int nblk;
  const int* hist;  // [M][hist_ld] generated tokens
  int hist_ld, gen_len;
  const int* banned;  // [M][hist_ld]
  const int* nbanned;
  float rep_penalty;
  int min_new, eos;
  int max_blocks;  // 0: one 16-column tile per workgroup; > 0: widen tiles to stay near this grid
  float* proc_out;  // EPI_LOGITS, optional [M, N]: the processed scores (sampling mode)
  int half;         // set by vcap_rows_gemm_dispatch: residual GEMV tiles split into two 8-column workgroups
  float* screen_h;  // lm_head stream kernel, optional [M, K] f32: workgroup 0 stores the ln_f rows it used
  // f32 K-split residual GEMV (vcap_rows_gemv8_kernel<float, NSL, true>): per (row chunk, tile) two
  // workgroups take one K half each; the pair meets through sk_part (2 x 256 f32 partials) and the
  // arrival ticket sk_cnt (zeroed by vcap_decode_init at the start of every decode)
  float* sk_part;
  int* sk_cnt;
  // EPI_QKV_ROWS: the row tables (device memory) in place of S_new / past
  const int* row_seq;  // [M] or nullptr (row m is sequence m)
  const int* row_pos;  // [M]
  int pos_add;
};

// Exact-fp32 greedy token from a bf16 lm_head screen (f32 decoders; vcap_decode_finalize_dispatch):
// the bf16 stream kernel left the processed approximate scores in `proc` [B][vocab], its argmax
// partials per block of `tpb` 16-column tiles, and the f32 ln_f rows in `sh` [B][E].  Every token
// whose exact f32 processed score could reach the approximate maximum's lower bound (|approx - exact|
// <= coef * ||h||, coef = c * max_v ||w_v|| * max(rep, 1 / rep)) is rescored against the f32 `w32`
// rows; the argmax of the exact scores (value, then lowest index) is the token.
struct ScreenArgs {
  const float* proc;
  const float* sh;
  const float* w32;
  float coef;
  int tpb;
  float rep;
  int min_new;
};

// ---- sampling warpers + draw (csrc/sample.hip)
struct SampleArgs {
  const float* proc;  // [rows][ldp] processed scores (processors applied)
  int V, ldp;
  float temperature;
  int top_k;
  double top_p;
  const unsigned* seed;  // device [2]: Philox key
  int step;
  const int* force;      // optional [rows][force_ld]: emit these tokens instead of drawing (tests)
  int force_ld;
  float* warped;         // optional [rows][warped_ld]: the warped scores HF's _sample draws from
  long warped_ld;
  float* pval;           // [rows]: the token as the finalize kernel's only argmax partial
  int* pidx;
  int eos;               // emitted for a row with no finite processed score (NaN / all -inf logits)
};
hipError_t vcap_sample_dispatch(const SampleArgs& a, int rows, hipStream_t s);
int vcap_sample_max_top_k();

hipError_t vcap_gemm_dispatch(int in_dt, int out_dt, const void* A, long lda, const void* W, long ldw, void* C,
                              long ldc, int M, int N, int K, const GemmEpi& epi, hipStream_t s);
int vcap_gemm_k_align(int in_dt);
// K splits (grid.y) of this thread's latest 128x128-kernel launch; 1 = unsplit
int vcap_gemm_last_splits();
// CUs a launch on stream s may use (its CU mask, else the device's CU count)
int vcap_stream_cus(hipStream_t s);
// CUs of the current device (launch plans that must not depend on a stream's CU mask)
int vcap_device_cus();
bool vcap_gemm256_ok(int in_dt, int out_dt, long lda, long ldw, long ldc, int M, int N, int K, const GemmEpi& epi);
hipError_t vcap_gemm256_dispatch(int in_dt, int out_dt, const void* A, long lda, const void* W, long ldw, void* C,
                                 long ldc, int M, int N, int K, const GemmEpi& epi, hipStream_t s);
void vcap_gemm_set_policy(int p);
hipError_t vcap_layernorm_mx_dispatch(const float* x, long ldx, uint8_t* q, uint8_t* scales, int srows,
                                      const float* gamma, const float* beta, int rows, int D, float eps,
                                      hipStream_t s);
hipError_t vcap_mx_quantize_dispatch(int in_dt, const void* x, long ldx, int rows, int K, uint8_t* q,
                                     uint8_t* scales, int srows, hipStream_t s);
hipError_t vcap_layernorm_dispatch(int out_dt, const float* x, long ldx, void* y, long ldy, const float* gamma,
                                   const float* beta, int rows, int D, float eps, hipStream_t s);
// whether vcap_vit_attention_dispatch has a kernel for N tokens of element type dt (the MXFP8-output form: dt = bf16)
bool vcap_vit_attention_supported(int dt, int N);
// cls_only: only the class-token query of each (frame, head), written to compact row `frame`
hipError_t vcap_vit_attention_dispatch(int dt, const void* qkv, void* out, int BT, int N, int H, hipStream_t s,
                                       int cls_only = 0);
// fused QKV projection + attention (bf16 or f16, 192 < N <= 208 or 256 < N <= 272): xn [BT*N, H*64] LayerNorm output, wqkv
// [3*H*64, H*64], bqkv [3*H*64] -> out as vcap_vit_attention_dispatch's
bool vcap_vit_qkv_attention_supported(int dt, int N, int H);
hipError_t vcap_vit_qkv_attention_dispatch(int dt, const void* xn, const void* wqkv, const float* bqkv, void* out,
                                           int BT, int N, int H, int cls_only, hipStream_t s);
hipError_t vcap_vit_attention_mx_dispatch(const void* qkv, void* out, uint8_t* oscale, int BT, int N, int H,
                                          hipStream_t s, int cls_only = 0);
hipError_t vcap_patchify_dispatch(int dt, const float* frames, void* patches, float* x, const float* cls,
                                  const float* pos, int BT, int img, int p, int Kp, int N, int D, hipStream_t s);
bool vcap_vit_head_prefix_supported(int D, int VD);
hipError_t vcap_vit_head_prefix_dispatch(const float* x, int B, int T, int N, int D, const float* ng, const float* nb,
                                         float neps, const float* pw, const float* pb, int VD, float ln_scale,
                                         float in_weight, const float* mw, const float* mb, int MO, float* enc_out,
                                         float* prefix, const float* emb_in, float* emb_scratch, hipStream_t s,
                                         int f16_head = 0);
hipError_t vcap_vit_pool_dispatch(int dt, const void* x, void* y, int B, int T, int tokens, int C, int gap,
                                  hipStream_t s);
hipError_t vcap_rows_gemm_dispatch(int dt, int pro, int epi, const RowsGemmArgs& a, int* nblk_out, hipStream_t s);
hipError_t vcap_rows_pack_dispatch(int dt, const void* w, long ldw, int N, int K, void* packed, hipStream_t s);
size_t vcap_rows_packed_size(int dt, int N, int K);
int vcap_logit_blocks(int V, int M);
// ---- decode attention (csrc/decode_attention.hip): S_new query rows per sequence, keys 0..past+i ----
// Where the keys of row m live, and which of them it may see.
struct DecodeKeys {
  // [seqs][maxp] page ids (maxp <= 64), or nullptr: the contiguous layout, page of position j of sequence
  // seq = seq * maxp + j / 16, which only contexts <= 64 take without a table
  const int* page_table = nullptr;
  // [M][anc_ld] (beam search; S_new == 1, no mask) or nullptr: key j of row m is position j of physical row
  // anc[m * anc_ld + j] of the contiguous layout; page_table is not read
  const int* anc = nullptr;
  int anc_ld = 0;
  // [seqs][mask_ld] bytes or nullptr: key j of a sequence with kmask[seq][j] == 0 is hidden from every query
  // of that sequence (score -inf before the softmax); key 0 must be visible
  const uint8_t* kmask = nullptr;
  int mask_ld = 0;
  // Ragged prompts: row m's query position from tables instead of (S_new, past) - sequence row_seq[m]
  // (nullptr: m), position row_pos[m] + pos_add.  The dispatcher is then called with S_new = 1 and
  // past + 1 = the longest sequence of the launch, min_len = the shortest; a sequence's length is
  // seq_len[seq] with row_seq (a packed prefill), else the row's own context.  Sequences of <= 64 run the
  // <= 64 form and longer ones the general form (what their one-prompt calls run).  No mask.
  const int* row_seq = nullptr;
  const int* row_pos = nullptr;
  int pos_add = 0;
  const int* seq_len = nullptr;
  int min_len = 0;
};
hipError_t vcap_decode_attention_dispatch(int dt, const void* q, const void* kc, const void* vc, const DecodeKeys& keys,
                                          int maxp, void* out, int M, int H, int S_new, int past, hipStream_t s);
// ---- teacher-forced scoring (csrc/score.hip): lm_head + cross-entropy over every row ----
struct ScoreLmArgs {
  const void* xn;       // [M][E] ln_f rows in the decoder dtype
  const void* wte;      // [V][E] tied lm_head, plain row-major (vcap_gpt2_desc.wte)
  int M, V, E;
  const int* targets;   // [M] or nullptr: token to predict at the row; outside [0, V) = ignored
  float* logits;        // [M][V] or nullptr
  float* part_max;      // [M][nparts]: per 64-column part, max and sum exp(x - max) of the row's logits
  float* part_sum;
  float* tgt_logit;     // [M]: the target's logit (written by the one part that holds its column)
  int nparts;           // vcap_score_parts(V)
};
int vcap_score_parts(int V);
hipError_t vcap_score_lm_dispatch(int dt, const ScoreLmArgs& a, hipStream_t s);
// log-prob of each row's target from the parts, in part order (0 where ignored; NaN for every row of a
// sequence whose key_mask[seq][0] is 0) -> logprob_ws [M] and, optional, logprob_out [M]; then, optional,
// loss_out = {sum of -logprob over the counted rows in row order, their count}
hipError_t vcap_score_combine_dispatch(const ScoreLmArgs& a, const uint8_t* kmask, int S, float* logprob_ws,
                                       float* logprob_out, float* loss_out, hipStream_t s);
// ---- the scoring call's backward (csrc/score_backward.hip): activation gradients, decoder dtype dt ----
// C f32 [M, ldc] = A [M, K] . W [N, K]^T with the 128x128 tile kernel at every M; N % 128 == 0, K a multiple of
// the K step.  k_per_slab > 0: K range z of that many columns goes to the slab C + z * M * ldc
// (ceil(K / k_per_slab) slabs).  vcap_grad_slab_sum_dispatch: out [n] = the slabs added in slab order, then
// + bias [N] (rows of N columns) and, round_bf16, rounded to bf16 values.
int vcap_grad_bk(int dt);   // the tile kernel's K step in elements: 32 f32, 64 bf16
hipError_t vcap_grad_gemm_dispatch(int dt, const void* A, long lda, const void* W, long ldw, float* C, long ldc,
                                   int M, int N, int K, int k_per_slab, hipStream_t s);
hipError_t vcap_grad_slab_sum_dispatch(const float* slabs, long n, int nslab, const float* bias, int N,
                                       int round_bf16, float* out, hipStream_t s);
// lse [M] from the score kernel's parts, then dl [M, Vpad] (dt) = w (1[v == target] - exp(logit - lse)); w == nullptr
// is -1; rows whose target is ignored and columns >= V are +0
hipError_t vcap_score_dlogit_dispatch(int dt, const float* part_max, const float* part_sum, int nparts,
                                      const float* logits, const int* targets, const float* w, int M, int V, int Vpad,
                                      float* lse, void* dl, hipStream_t s);
// g [M, E] += the LayerNorm input gradient of dy at the rows x (gamma frozen)
hipError_t vcap_ln_backward_dispatch(const float* x, const float* dy, const float* gamma, float eps, int M, int E,
                                     float* g, hipStream_t s);
// the same update of g (same bits), plus stats [M][2] = each row's (mean, rstd) for vcap_ln_colsum_dispatch
hipError_t vcap_ln_backward_stats_dispatch(const float* x, const float* dy, const float* gamma, float eps, int M,
                                           int E, float* g, float* stats, hipStream_t s);
// dW [K, N] f32 = X^T . dY over the M <= 512 rows of X [M, K] and dY [M, N] (dt); K % 64 == 0, N % 128 == 0
// (gpt2_weight_grad.hip)
hipError_t vcap_gpt2_dw_dispatch(int dt, const void* X, const void* dY, float* dW, int M, int K, int N,
                                 hipStream_t s);
hipError_t vcap_gelu_backward_dispatch(int dt, const float* u, const float* dact, long n, void* du, hipStream_t s);
hipError_t vcap_grad_to_bf16_dispatch(const float* x, long n, void* y, hipStream_t s);
// qkv [B*S, 3 * 64 H] f32, dO [B*S, 64 H] f32, kmask [B, S] or nullptr; P, dS: [B*H, S, S] f32 scratch;
// dqkv [B*S, 3 * 64 H] (dt).  S <= 512.
hipError_t vcap_attn_backward_dispatch(int dt, const float* qkv, const float* dO, const uint8_t* kmask, int B, int S,
                                       int H, float* P, float* dS, void* dqkv, hipStream_t s);
// out = g + 0; NaN for the rows of a sequence with kmask[seq][0] == 0
hipError_t vcap_grad_finish_dispatch(const float* g, const uint8_t* kmask, int B, int S, int E, float* out,
                                     hipStream_t s);
hipError_t vcap_prefill_embed_dispatch(int dt, const float* prefix, int P, const int* ids, int nids, const void* wte,
                                       const float* wpe, float* h, int B, int E, hipStream_t s, int pos0 = 0,
                                       int prefix_rep = 1);
// Ragged prompts (device tables): rows row_seq[m] / row_pos[m] of a packed prefill; sequence r's prefix is
// prefix[r / prefix_rep], its prompt ids[ids_off[r / prefix_rep] + (i - P)]
hipError_t vcap_prefill_embed_rows_dispatch(int dt, const float* prefix, int P, const int* ids, const int* ids_off,
                                            const int* row_seq, const int* row_pos, const void* wte, const float* wpe,
                                            float* h, int M, int E, int prefix_rep, hipStream_t s);
// dst[r] = src[rows[r]] (f32 rows of E): each sequence's last prefill row, for the lm_head
hipError_t vcap_gather_rows_dispatch(const float* src, const int* rows, float* dst, int R, int E, hipStream_t s);
hipError_t vcap_decode_init_dispatch(int* page_table, int B, int maxp, int* finished, int* nbanned, hipStream_t s,
                                     int* sk_cnt = nullptr, int n_sk = 0);
hipError_t vcap_decode_finalize_dispatch(int dt, const float* part_val, const int* part_idx, int nblk, int B,
                                         int step, int* finished, int* hist, int hist_ld, int* banned, int* nbanned,
                                         int ngram, int eos, int pad, int* out_ids, int out_ld, const void* wte,
                                         const float* wpe, float* h, int E, int pos_next, int vocab, hipStream_t s,
                                         const ScreenArgs* screen = nullptr);
// Ragged prompts: the next input's position is min(seq_len[m] + pos_add, npos - 1) per row
hipError_t vcap_decode_finalize_rows_dispatch(int dt, const float* part_val, const int* part_idx, int nblk, int B,
                                              int step, int* finished, int* hist, int hist_ld, int* banned,
                                              int* nbanned, int ngram, int eos, int pad, int* out_ids, int out_ld,
                                              const void* wte, const float* wpe, float* h, int E, const int* seq_len,
                                              int pos_add, int npos, int vocab, hipStream_t s,
                                              const ScreenArgs* screen = nullptr);
// The bf16 lm_head as the screen of an f32 greedy step (the stream kernel only: M <= 16); returns
// hipErrorNotSupported, launching nothing, where that kernel does not apply.
hipError_t vcap_lm_head_screen_dispatch(const RowsGemmArgs& a, int* nblk_out, int* tpb_out, hipStream_t s);
hipError_t vcap_embed_tokens_dispatch(int dt, const int* tok, int rows, const void* wte, const float* wpe, float* h,
                                      int E, int pos, hipStream_t s);
// ... at position min(seq_len[r] + pos_add, npos - 1) per row (ragged beam search)
hipError_t vcap_embed_tokens_rows_dispatch(int dt, const int* tok, int rows, const void* wte, const float* wpe,
                                           float* h, int E, const int* seq_len, int pos_add, int npos, hipStream_t s);
// ---- device beam search (csrc/beam.hip) ----
struct BeamState {  // per-call device state, carved from the caller's workspace (B batches, nb beams, L = max_new)
  int* run_seq;      // [B][nb][L] running hypotheses' tokens
  float* run_score;  // [B][nb]
  int* run_bidx;     // [B][nb][L] beam indices (HF running_beam_indices)
  int* seqs;         // [B][nb][L] finished hypotheses (EOS-initialised)
  float* beam_score; // [B][nb] (-1e9 initialised)
  int* beam_idx;     // [B][nb][L] (-1 initialised)
  int* fin;          // [B][nb]
  int* unsat;        // [B]
  int* stopped;      // [1] HF's loop has ended (no further updates)
  int* tok_next;     // [B*nb] next input tokens
  int* anc;          // [B*nb][anc_ld] physical row holding each position's K/V
  float* cand_val;   // [B*nb][C][2nb]
  int* cand_tok;
};
hipError_t vcap_beam_init_dispatch(const BeamState& st, int B, int nb, int L, int S0, int anc_ld, int eos,
                                   hipStream_t s);
hipError_t vcap_beam_cand_dispatch(const BeamState& st, const float* logits, const float* part_max,
                                   const float* part_sum, int nblk, int rows, int V, int nb, int L, int cur,
                                   float rep, int ngram, int min_new, int eos, int chunks, hipStream_t s);
hipError_t vcap_beam_select_dispatch(const BeamState& st, int B, int nb, int L, int V, int chunks, int cur, int eos,
                                     float length_penalty, int S0, int anc_ld, hipStream_t s,
                                     const int* seq_len = nullptr);  // seq_len [B * nb]: S0 of batch b = seq_len[b * nb]
hipError_t vcap_beam_output_dispatch(const BeamState& st, int B, int nb, int L, int* out_ids, int* out_len,
                                     hipStream_t s);
int vcap_beam_chunks(int V);

hipError_t vcap_kv_gather_dispatch(int dt, const void* src_pool, void* dst_pool, const int* src_rows, int rows, int maxp,
                                   int H, int len, long layer_elems, int L, hipStream_t s);
size_t vcap_frames_ws_bytes(int n, int in_h, int in_w, int out_h, int out_w);
hipError_t vcap_frames_preprocess_dispatch(const uint8_t* frames, int n, int in_h, int in_w, int out_h, int out_w,
                                           const float* mean3, const float* std3, float* out, uint8_t* out_u8,
                                           void* ws, hipStream_t s);

// ---- video retrieval (csrc/retrieval.hip): L2 normalisation, index storage conversion, flat-IP top-k ----
constexpr int kIpSlabRows = 128;           // database rows a scan workgroup takes per step
constexpr int kIpMaxK = 128;
constexpr int kIpMaxWorkgroups = 512;      // scan grid cap (the workspace is sized for it)
constexpr int kIpMaxQueryFloats = 16384;   // nq * dim of one call; one scan launch holds 16-query tiles of it in LDS
int vcap_ip_search_cap(int k);                      // keys per (workgroup, query) workspace buffer
int vcap_ip_search_grid(long n, int max_blocks);    // scan workgroups for n rows
int vcap_ip_search_pass_tiles(int dim);             // 16-query tiles per scan launch (more queries: more passes)
hipError_t vcap_ip_search_dispatch(int dt, const void* db, long n, int dim, const float* queries, int nq, int k,
                                   float* out_scores, long long* out_ids, void* workspace, int max_blocks,
                                   hipStream_t s);
hipError_t vcap_l2_normalize_dispatch(const float* x, long ldx, float* y, long ldy, int rows, int dim, float eps,
                                      int eps_mode, hipStream_t s);
hipError_t vcap_ip_convert_dispatch(int dt, const float* x, long ldx, long rows, int dim, void* dst, hipStream_t s);
// the flat search's merge alone: the k best of ws[list][query][0, k) (keys, row stride cap) -> the outputs
hipError_t vcap_ip_merge_dispatch(const void* ws, int lists, int nq, int cap, int k, float* out_scores,
                                  long long* out_ids, hipStream_t s);

// ---- IVF-Flat index (csrc/ivf.hip): coarse assignment, spherical centroid update, probed list scan ----
constexpr int kIvfSliceRows = 512;         // rows of one list a scan workgroup takes: an item is (query, probe, slice)
constexpr int kIvfChunkRows = 512;         // member rows one wave sums in the centroid update
constexpr int kIvfMaxProbe = 128;
constexpr int kIvfMaxLists = 1 << 20;
// assign[r] = the centroid with the largest inner product (lowest id on ties, -1 when every score is NaN),
// score[r] (optional) that score: the bits vcap_ip_search_dispatch(db = centroids, queries = row) returns
hipError_t vcap_ivf_assign_dispatch(const float* x, long ldx, long n, const float* centroids, int nlist, int dim,
                                    int* assign, float* score, hipStream_t s);
long vcap_ivf_update_slots(long n, int nlist);   // partial-sum rows of the centroid update's workspace
hipError_t vcap_ivf_centroid_update_dispatch(const float* x, long ldx, long n, int dim, const long long* order,
                                             const long long* offsets, int nlist, const float* prev, float* out,
                                             float eps, float* partials, hipStream_t s);
// probes [nq, nprobe] / probe_scores: the coarse stage's outputs; keys: [nprobe * slices][nq][k] 8-byte slots
hipError_t vcap_ivf_search_dispatch(int dt, const void* rows, const long long* ids, const long long* offsets, long ntotal,
                                    const float* centroids, int nlist, long max_list_len, int dim,
                                    const float* queries, int nq, int nprobe, int k, float* out_scores,
                                    long long* out_ids, long long* probes, float* probe_scores, void* coarse_ws,
                                    void* keys, int max_blocks, hipStream_t s);

// ---- text tower (csrc/text_encoder.hip): M = B * L rows of E = 64 H features, L <= 64 ----
// x (f32) and xt (T) [M, E] = emb[ids]; an id outside [0, vocab) gives a NaN row
hipError_t vcap_text_gather_dispatch(int dt, const int* ids, int M, const float* emb, int vocab, int E, float* x,
                                     void* xt, hipStream_t s);
// qkv T [M, 3E] (q | k | v) -> out T [M, E]: softmax(q k^T / 8) v per (caption, head), no mask
hipError_t vcap_text_attention_dispatch(int dt, const void* qkv, void* out, int B, int L, int H, hipStream_t s);
// x <- LayerNorm(x) in place (f32) and its T copy xt; E % 128 == 0, E <= 1024
hipError_t vcap_text_resid_ln_dispatch(int dt, float* x, void* xt, const float* gamma, const float* beta, int M, int E,
                                       float eps, hipStream_t s);
// out [B, P] = normalize(pw . mean over ids != pad of x + pb), eps 1e-12; P % 64 == 0, 64 <= P <= 1024
hipError_t vcap_text_pool_dispatch(const float* x, const int* ids, int pad_id, int B, int L, int E, const float* pw,
                                   const float* pb, int P, float* out, hipStream_t s);

// ---- text tower backward (csrc/text_backward.hip): parameter gradients, f32 outputs, fixed orders ----
// dy [B, P], pooled [B, E] and g [M, E] (the gradient at the encoder output) from gout [B, P] at the forward's
// out; then dproj_w [P, E] and dproj_b [P], captions in order
hipError_t vcap_text_tail_bwd_dispatch(const float* x, const int* ids, int pad_id, int B, int L, int E,
                                       const float* pw, const float* pb, int P, const float* out, const float* gout,
                                       float* dy, float* pooled, float* g, float* dproj_w, float* dproj_b,
                                       hipStream_t s);
// dx [M, E] = the LayerNorm input gradient of dy = a (+ b; b may be null) at the rows x; a <- dy; stats [M, 2];
// dgamma, dbeta [E] summed over the rows in a fixed order
hipError_t vcap_text_ln_bwd_dispatch(const float* x, float* a, const float* b, const float* gamma, float eps, int M,
                                     int E, float* dx, float* stats, float* dgamma, float* dbeta, hipStream_t s);
// out [N] = sum over the M rows of src [M, N] in a fixed order; N % 64 == 0
hipError_t vcap_text_colsum_dispatch(const float* src, int M, int N, float* out, hipStream_t s);
// the same sum over rows of dtype dt (f32 or bf16), f32 accumulation and output
hipError_t vcap_colsum_dispatch(int dt, const void* src, int M, int N, float* out, hipStream_t s);
// dgamma [E] = sum_m dy[m] xhat[m] and dbeta [E] = sum_m dy[m] in the column sum's order; xhat from the rows x
// and their stats [M][2] = (mean, rstd)
hipError_t vcap_ln_colsum_dispatch(const float* dy, const float* x, const float* stats, int M, int E, float* dgamma,
                                   float* dbeta, hipStream_t s);
// dst (dt) [N, Mpad] = src^T, src [M, N] f32 (src_f32) or dt; columns m >= M are +0; N % 64 == 0, Mpad % 32 == 0
hipError_t vcap_text_transpose_dispatch(int dt, int src_f32, const void* src, int M, int N, int Mpad, void* dst,
                                        hipStream_t s);
// d [n] <- d where act (dt) > 0, else +0
hipError_t vcap_text_relu_bwd_dispatch(int dt, const void* act, long n, float* d, hipStream_t s);
// qkv (dt) [B*L, 3 * 64 H], dO f32 [B*L, 64 H]; P, dS: [B*H, L, L] f32 scratch; dqkv f32 [B*L, 3 * 64 H]; no mask
hipError_t vcap_text_attn_bwd_dispatch(int dt, const void* qkv, const float* dO, int B, int L, int H, float* P,
                                       float* dS, float* dqkv, hipStream_t s);
// the row-sparse embedding gradient of dx0 = a (+ b): slot [M] scratch, emb_ids [M], count [1], rows [M, E]; M <= 512
hipError_t vcap_text_emb_grad_dispatch(const int* ids, int M, int pad_id, int vocab, const float* a, const float* b,
                                       int E, int* slot, int* emb_ids, int* count, float* rows, hipStream_t s);

// ---- ViT backward (csrc/vit_backward.hip): parameter gradients of the encoder, f32 outputs, fixed orders ----
// C [K, N] f32 = sum over rows of X[row][k] Y[row][n], X [rows, Kmem >= K] and Y [rows, N] row-major in dt (f32 or
// bf16).  Launch batch z = (z1, z2) = (z / Z2, z % Z2) takes rows [0, min(slab_rows, rows_total - z1 * slab_step))
// of X + z1 xs1 + z2 xs2 and Y + z1 ys1 + z2 ys2 into C + z1 cs1 + z2 cs2 (offsets in elements).
struct XtyArgs {
  const void* X;
  long ldx;
  int Kmem;
  const void* Y;
  long ldy;
  int N;
  float* C;
  long ldc;
  int K;
  int rows_total, slab_rows, slab_step;
  int Z2;
  long xs1, xs2, ys1, ys2, cs1, cs2;
};
hipError_t vcap_vit_xty_dispatch(int dt, const XtyArgs& a, int Z, hipStream_t s);
// row stride (and row count) of one (frame, head)'s P / dS / dS^T scratch matrix: N rounded up to 64
int vcap_vit_attn_bwd_ldp(int N);
// qkv (dt) [BT*N, 3 * 64 H], dO (dt) [BT*N, 64 H]; P, dS, dST: [BT*H][ldp][ldp] dt scratch; dqkv f32
// [BT*N, 3 * 64 H].  1 <= N <= 288.
hipError_t vcap_vit_attn_bwd_dispatch(int dt, const void* qkv, const void* dO, int BT, int N, int H, void* P, void* dS,
                                      void* dST, float* dqkv, hipStream_t s);
// xn [B*T, D]: the final norm of the CLS rows.  pooled [B, D], dn [B*T, D] = (gout . pw) / T, then dproj_w [VD, D]
// and dproj_b [VD], videos in order
hipError_t vcap_vit_head_bwd_dispatch(const float* xn, int B, int T, int D, const float* gout, const float* pw, int VD,
                                      float* pooled, float* dn, float* dproj_w, float* dproj_b, hipStream_t s);
// dpos [N, D] = sum over the BT frames in order of g [BT*N, D]; dcls [D] = dpos[0]
hipError_t vcap_vit_pos_grad_dispatch(const float* g, int BT, int N, int D, float* dpos, float* dcls, hipStream_t s);
// dst[r * ldd + i] = src[r * lds + i] for r < rows, i < width (f32)
hipError_t vcap_vit_rows_copy_dispatch(const float* src, long lds, float* dst, long ldd, int rows, long width,
                                       hipStream_t s);

// JPEG frame decode (jpeg.hip): header of one baseline image, workspace of n same-shape images,
// host entropy decode + device IDCT / upsampling / colour conversion into uint8 [n, H, W, 3].
struct JpegInfo {
  int width = 0, height = 0, ncomp = 0, hmax = 1, vmax = 1;
  int id[3] = {0, 0, 0}, h[3] = {1, 1, 1}, v[3] = {1, 1, 1};
  int bx[3] = {0, 0, 0}, by[3] = {0, 0, 0};  // block grid per component, padded to whole MCUs
};
int vcap_jpeg_header(const uint8_t* data, size_t len, JpegInfo* info, std::string* err);
size_t vcap_jpeg_ws_bytes(const JpegInfo& f, int n);
int vcap_jpeg_decode(const uint8_t* const* data, const size_t* lens, int n, uint8_t* out, void* ws, size_t ws_bytes,
                     hipStream_t s, std::string* err);
// The host stage of vcap_jpeg_decode alone (no device call; tools/jpeg_host_check.cpp runs it under the
// host sanitizers): parse n images of one shape into *info, then entropy-decode them into the buffer
// `stage` returns for (shape, bytes = vcap_jpeg_stage_bytes): the int16 coefficients, then from the next
// 16-byte boundary the images' quantisation tables [image][component][64].  A null buffer ends the call
// with the *rc / *err the allocator set.
using JpegStageAlloc = std::function<void*(const JpegInfo& f, size_t bytes, int* rc, std::string* err)>;
size_t vcap_jpeg_stage_bytes(const JpegInfo& f, int n);
int vcap_jpeg_host_stage(const uint8_t* const* data, const size_t* lens, int n, JpegInfo* info,
                         const JpegStageAlloc& stage, std::string* err);
