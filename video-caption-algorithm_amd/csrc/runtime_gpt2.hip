// The GPT-2 side of the C ABI (include/vcap.h): descriptor and prompt checks, the decode state carved
// from the caller's workspace, the layer schedule, and the entry points built on it - greedy and sampling
// decode (one hipGraph, graph_cache.hip), device beam search, the prefill / step / reorder calls of the
// host-bookkeeping search, and teacher-forced scoring.
//
// The reference drives these steps from Python (HF generate); here the whole schedule is native so one
// ABI call issues the full decode (~60 launches per token), captured once into a hipGraph and replayed.
#include <algorithm>
#include <vector>

#include "runtime_common.h"

namespace {

// Decoder rows one call may carry (B * (prefix + prompt) at the prefill, rows of a step).  Rows go
// through the GEMV kernels in 16 / 32-row chunks (blockIdx.y), so this bounds workspace sizes only.
constexpr int kMaxDecodeRows = 512;

// Decode state of `B` rows carved from a workspace (carve_dec)
struct DecState {
  int maxp;           // KV pages per row
  size_t page_elems;  // elements of one layer's K (or V) pool
  float* h;
  float* sh;  // [B][E] f32 ln_f rows of the bf16 lm_head screen (f32 greedy)
  void* q;
  void* attn;
  void* act;
  void* kc;
  void* vc;
  int* pt;
  float* pval;
  int* pidx;
  int* hist;
  int* banned;
  int* nbanned;
  int* finished;
  float* proc;        // [B][V] processed scores (sampling mode)
  unsigned* seed;     // [2] Philox key of the sampling draws
  // f32 mlp c_proj K split (RowsGemmArgs.sk_*): pair partials + tickets, zeroed by vcap_decode_init at
  // the start of every decode, prefill and forward_embeds sequence (all f32 paths run the same split,
  // so a teacher-forced forward reproduces the free-running graph's logits bit for bit)
  float* skp;
  int* skc;
  int n_skc;
};

int max_logit_blocks(int V, int B) { return vcap_logit_blocks(V, B); }

// prefill_rows > 0 (ragged prompts): the prefill packs that many rows instead of B * S0, and S0 (the
// longest sequence's) sizes the pages only
DecState carve_dec(Carver& c, const vcap_gpt2_desc* d, int B, int S0, int max_new, int prefill_rows = 0) {
  const int E = d->n_embd;
  const size_t es = esize(d->dtype);
  const size_t M0 = prefill_rows > 0 ? (size_t)prefill_rows : (size_t)B * S0;
  const size_t Mmax = M0 > (size_t)B ? M0 : B;
  DecState b;
  b.maxp = (S0 + max_new + 15) / 16;
  const size_t pages = (size_t)B * b.maxp;
  b.page_elems = pages * d->n_head * 16 * 64;
  b.h = (float*)c.take(Mmax * E * 4);
  b.q = c.take(Mmax * E * es);
  b.attn = c.take(Mmax * E * es);
  b.act = c.take(Mmax * 4 * E * es);
  b.kc = c.take(b.page_elems * d->n_layer * es);
  b.vc = c.take(b.page_elems * d->n_layer * es);
  b.pt = (int*)c.take(pages * 4);
  // argmax partials: the lm_head's 64-column GEMV blocks or its stream kernel's grid (<= CUs)
  const int nb = std::max({max_logit_blocks(d->vocab, B), vcap_device_cus(), 256});
  b.pval = (float*)c.take((size_t)B * nb * 4);
  b.pidx = (int*)c.take((size_t)B * nb * 4);
  b.hist = (int*)c.take((size_t)B * max_new * 4);
  b.banned = (int*)c.take((size_t)B * max_new * 4);
  b.nbanned = (int*)c.take((size_t)B * 4);
  b.finished = (int*)c.take((size_t)B * 4);
  b.proc = (float*)c.take((size_t)B * d->vocab * 4);
  b.sh = (float*)c.take((size_t)B * E * 4);
  b.seed = (unsigned*)c.take(8);
  // K split: every 16-row chunk of the largest launch (Mmax rows) x E / 16 tiles x 256 partials x 4
  // (the pairs: 2 halves per tile; the f32 4-way split: E / 32 groups x 4 parts x 2 tiles); the
  // tickets, one per tile or group
  b.n_skc = (int)((Mmax + 15) / 16) * ((E + 15) / 16);
  b.skp = (float*)c.take((size_t)b.n_skc * 4 * 256 * 4);
  b.skc = (int*)c.take((size_t)b.n_skc * 4);
  return b;
}

int check_gpt2(const vcap_gpt2_desc* d) {
  if (!d || !d->layers) return fail(VCAP_E_ARG, "gpt2 desc is null");
  if (d->dtype != VCAP_DT_F32 && d->dtype != VCAP_DT_BF16) return fail(VCAP_E_ARG, "gpt2 dtype");
  if (d->n_head * 64 != d->n_embd) return fail(VCAP_E_UNSUPPORTED, "gpt2 head_dim must be 64");
  if (d->n_embd % 128) return fail(VCAP_E_UNSUPPORTED, "n_embd must be a multiple of 128");
  if (d->n_embd > 1024) return fail(VCAP_E_UNSUPPORTED, "n_embd > 1024 (LayerNorm rows are held in registers)");
  return 0;
}

// shape checks + the weight pointers a launch dereferences
int check_gpt2_launch(const vcap_gpt2_desc* d) {
  if (int rc = check_gpt2(d)) return rc;
  if (!d->lm_head || !d->wte || !d->wpe || !d->lnf_g || !d->lnf_b)
    return fail(VCAP_E_ARG, "gpt2 wte / lm_head / wpe / ln_f pointer is null");
  return 0;
}

// The prompt checks of generate / sample / beam_search / prefill.  Each entry point has checks of its
// own between these (with its own messages), so they come in pieces called in that entry point's order.
int check_prompt_args(const char* name, const float* prefix, const int* prompt_ids, int prompt_len, int B) {
  if (!prefix || B <= 0 || prompt_len < 0 || prompt_len > 64 || (prompt_len && !prompt_ids))
    return fail(VCAP_E_ARG, std::string(name) + ": bad arguments");
  return 0;
}

int check_prompt_ids(const vcap_gpt2_desc* d, const int* prompt_ids, int prompt_len) {
  for (int i = 0; i < prompt_len; ++i)
    if (prompt_ids[i] < 0 || prompt_ids[i] >= d->vocab) return fail(VCAP_E_ARG, "prompt id out of range");
  return 0;
}

// greedy and sampling decode: B sequences of prefix + prompt rows, max_new (<= 64) more positions
int check_prompt_rows(const vcap_gpt2_desc* d, const int* prompt_ids, int prompt_len, int B, int max_new) {
  const int S0 = d->prefix_len + prompt_len;
  if (S0 <= 0 || B * S0 > kMaxDecodeRows)
    return fail(VCAP_E_UNSUPPORTED, "B*(prefix+prompt) exceeds vcap_gpt2_max_rows()");
  if (S0 + max_new > d->n_positions) return fail(VCAP_E_UNSUPPORTED, "context exceeds n_positions");
  return check_prompt_ids(d, prompt_ids, prompt_len);
}

// beam search: keys through the ancestry table (one query row per sequence); teacher-forced scoring:
// keys hidden per sequence on top of the causal order
struct LayerExtras {
  const int* anc = nullptr;
  int anc_ld = 0;
  const uint8_t* kmask = nullptr;
  int mask_ld = 0;
  // ragged prompts: row m is position row_pos[m] + pos_add of sequence row_seq[m] (nullptr: m); run_layers
  // is then called with S_new = 1 and past + 1 = the largest context of the launch
  const int* row_seq = nullptr;
  const int* row_pos = nullptr;
  int pos_add = 0;
  const int* seq_len = nullptr;   // [seqs], with row_seq
  int min_len = 0;                // the shortest sequence of the launch (past + 1 is the longest)
  // the scoring call's backward (host only: copies between the launches, which stay as they are): the f32
  // residual stream [M, E] is copied to snap + 2 l * M * E at layer l's input, to snap + (2 l + 1) * M * E
  // after its attention c_proj and to snap + 2 L * M * E at the last layer's output
  float* snap = nullptr;
  // the tail call's weight gradients (also host only): in the layers l >= tail->first_layer the attention
  // output [M, E] and the c_fc output after gelu_new [M, 4E], both in the decoder dtype, are copied to
  // tail->att / tail->act + (l - first_layer) * their size right after the launch that wrote them
  const ScoreTailSnap* tail = nullptr;
};

int run_layers(const vcap_gpt2_desc* d, const DecState& w, int M, int S_new, int past, int max_blocks, hipStream_t s,
               const LayerExtras& x = {}) {
  const int E = d->n_embd, H = d->n_head, L = d->n_layer;
  const int dt = d->dtype;
  const size_t es = esize(dt);
  const size_t snap_n = (size_t)M * E;
  for (int l = 0; l < L; ++l) {
    const vcap_gpt2_layer& ly = d->layers[l];
    if (x.snap)
      VCAP_TRY(hipMemcpyAsync(x.snap + 2 * l * snap_n, w.h, snap_n * 4, hipMemcpyDeviceToDevice, s), "snapshot");
    RowsGemmArgs a{};
    a.M = M;
    a.ln_eps = d->ln_eps;
    // 1) ln_1 + c_attn -> q, paged K/V
    a.x = w.h; a.ldx = E; a.ln_g = ly.ln1_g; a.ln_b = ly.ln1_b;
    a.w = ly.attn_w; a.bias = ly.attn_b; a.N = 3 * E; a.K = E;
    a.q_out = w.q;
    a.kc = (char*)w.kc + (size_t)l * w.page_elems * es;
    a.vc = (char*)w.vc + (size_t)l * w.page_elems * es;
    // pages are allocated contiguously per sequence (identity table written by vcap_decode_init):
    // the scatter computes page ids instead of loading them (nullptr table)
    a.page_table = nullptr; a.maxp = w.maxp; a.H = H; a.S_new = S_new; a.past = past; a.max_blocks = max_blocks;
    a.row_seq = x.row_seq; a.row_pos = x.row_pos; a.pos_add = x.pos_add;
    VCAP_TRY(vcap_rows_gemm_dispatch(dt, PRO_LN, x.row_pos ? EPI_QKV_ROWS : EPI_QKV, a, nullptr, s), "c_attn");
    // 2) causal attention over the paged cache
    // pages are allocated contiguously per sequence (vcap_decode_init: identity table), so the
    // short-context kernels (bf16 and f32) compute page ids instead of loading them (nullptr table);
    // beam search reads through its ancestry table instead
    const DecodeKeys keys{x.anc || past + S_new <= 64 ? nullptr : w.pt, x.anc, x.anc_ld, x.kmask, x.mask_ld,
                          x.row_seq, x.row_pos, x.pos_add, x.seq_len, x.min_len};
    VCAP_TRY(vcap_decode_attention_dispatch(dt, w.q, a.kc, a.vc, keys, w.maxp, w.attn, M, H, S_new, past, s),
             "decode_attention");
    const bool keep = x.tail && l >= x.tail->first_layer;
    if (keep)
      VCAP_TRY(hipMemcpyAsync((char*)x.tail->att + (size_t)(l - x.tail->first_layer) * snap_n * es, w.attn,
                              snap_n * es, hipMemcpyDeviceToDevice, s),
               "snapshot");
    // 3) attn c_proj + residual
    RowsGemmArgs b{};
    b.M = M; b.x = w.attn; b.ldx = E; b.w = ly.aproj_w; b.bias = ly.aproj_b; b.N = E; b.K = E;
    b.out = w.h; b.ldo = E; b.max_blocks = max_blocks;
    VCAP_TRY(vcap_rows_gemm_dispatch(dt, PRO_DIRECT, EPI_RESID, b, nullptr, s), "attn_c_proj");
    if (x.snap)
      VCAP_TRY(hipMemcpyAsync(x.snap + (2 * l + 1) * snap_n, w.h, snap_n * 4, hipMemcpyDeviceToDevice, s), "snapshot");
    // 4) ln_2 + c_fc + gelu_new
    RowsGemmArgs c{};
    c.M = M; c.x = w.h; c.ldx = E; c.ln_g = ly.ln2_g; c.ln_b = ly.ln2_b; c.ln_eps = d->ln_eps;
    c.w = ly.fc_w; c.bias = ly.fc_b; c.N = 4 * E; c.K = E; c.out = w.act; c.ldo = 4 * E; c.max_blocks = max_blocks;
    VCAP_TRY(vcap_rows_gemm_dispatch(dt, PRO_LN, EPI_GELU, c, nullptr, s), "c_fc");
    if (keep)
      VCAP_TRY(hipMemcpyAsync((char*)x.tail->act + (size_t)(l - x.tail->first_layer) * 4 * snap_n * es, w.act,
                              4 * snap_n * es, hipMemcpyDeviceToDevice, s),
               "snapshot");
    // 5) mlp c_proj + residual, K split at every row count: the arithmetic may not depend on the
    // launch's M (the dispatcher drops the split where it does not apply)
    RowsGemmArgs e{};
    e.M = M; e.x = w.act; e.ldx = 4 * E; e.w = ly.mproj_w; e.bias = ly.mproj_b; e.N = E;
    e.K = 4 * E; e.out = w.h; e.ldo = E; e.max_blocks = max_blocks;
    e.sk_part = w.skp; e.sk_cnt = w.skc;
    VCAP_TRY(vcap_rows_gemm_dispatch(dt, PRO_DIRECT, EPI_RESID, e, nullptr, s), "mlp_c_proj");
  }
  if (x.snap)
    VCAP_TRY(hipMemcpyAsync(x.snap + 2 * L * snap_n, w.h, snap_n * 4, hipMemcpyDeviceToDevice, s), "snapshot");
  return 0;
}

// ln_f on each sequence's last row (fused into the A prologue) + the tied lm_head over `rows`
// sequences of S_new rows each: what every lm_head launch has in common
RowsGemmArgs lm_head_args(const vcap_gpt2_desc* d, const DecState& w, int rows, int S_new) {
  const int E = d->n_embd;
  RowsGemmArgs g{};
  g.M = rows; g.x = w.h + (size_t)(S_new - 1) * E; g.ldx = (long)S_new * E;
  g.ln_g = d->lnf_g; g.ln_b = d->lnf_b; g.ln_eps = d->ln_eps;
  g.w = d->lm_head; g.N = d->vocab; g.K = E;
  return g;
}

// ... plus the argmax partials it leaves and the processors' state (EPI_LOGITS and the screen)
RowsGemmArgs logits_args(const vcap_gpt2_desc* d, const DecState& w, int rows, int S_new, int hist_ld, int gen_len) {
  RowsGemmArgs g = lm_head_args(d, w, rows, S_new);
  g.part_val = w.pval; g.part_idx = w.pidx;
  g.hist = w.hist; g.hist_ld = hist_ld; g.gen_len = gen_len; g.banned = w.banned; g.nbanned = w.nbanned;
  return g;
}

// prefill / step / forward_embeds: the layers over `rows` sequences of S_new new rows each, then the
// raw logits of each sequence's last row (no processors)
int run_raw_forward(const vcap_gpt2_desc* d, const DecState& w, int rows, int S_new, int past, float* logits_out,
                    hipStream_t s) {
  if (int rc = run_layers(d, w, rows * S_new, S_new, past, 0, s)) return rc;
  RowsGemmArgs g = logits_args(d, w, rows, S_new, 1, 0);
  g.logits_raw = logits_out;
  g.nblk = max_logit_blocks(d->vocab, rows);
  g.rep_penalty = 1.0f; g.eos = -1;
  int nblk;
  VCAP_TRY(vcap_rows_gemm_dispatch(d->dtype, PRO_LN, EPI_LOGITS, g, &nblk, s), "lm_head");
  return 0;
}

// ---- ragged prompts: B prompts of their own lengths in one decode.  R = B * rep row-sequences (rep =
// num_beams for the search's replicated prefill, else 1); sequence r carries prompt r / rep and
// S0[r / rep] = prefix_len + len positions; the prefill packs the sequences' rows back to back.
struct Ragged {
  int B = 0, rep = 1, R = 0, M = 0, nids = 0, max_S0 = 0, min_S0 = 0;
  const int* offsets = nullptr;  // host [B + 1]
  // device, carved from the workspace: one int block [row_seq M | row_pos M | seq_len R | last_row R |
  // ids_off B | ids nids] (uploaded in one copy) and the gathered last prefill rows
  int* tab = nullptr;
  float* hl = nullptr;
  int* row_seq() const { return tab; }
  int* row_pos() const { return tab + M; }
  int* seq_len() const { return tab + 2 * M; }
  int* last_row() const { return tab + 2 * M + R; }
  int* ids_off() const { return tab + 2 * M + 2 * R; }
  int* ids() const { return tab + 2 * M + 2 * R + B; }
  size_t tab_ints() const { return (size_t)2 * M + 2 * R + B + nids; }
};

// The shape checks every ragged entry point and workspace query share (the limits in include/vcap.h).
// s0_zero_code: what an empty sequence is (the uniform generate / beam search: UNSUPPORTED, sample: ARG).
int ragged_shape(const char* name, const vcap_gpt2_desc* d, const int* offsets, int B, int max_new, int rep,
                 int s0_zero_code, Ragged* out) {
  if (!offsets || B <= 0 || offsets[0] != 0) return fail(VCAP_E_ARG, std::string(name) + ": bad arguments");
  Ragged r;
  r.B = B; r.rep = rep; r.R = B * rep; r.offsets = offsets;
  long M = 0;
  for (int b = 0; b < B; ++b) {
    const long len = (long)offsets[b + 1] - offsets[b];
    if (len < 0) return fail(VCAP_E_ARG, std::string(name) + ": prompt offsets must be non-decreasing");
    if (len > 64) return fail(VCAP_E_ARG, std::string(name) + ": bad arguments (a prompt over 64 ids)");
    const int S0 = d->prefix_len + (int)len;
    if (S0 <= 0) return fail(s0_zero_code, std::string(name) + ": a sequence with no prefix and no prompt");
    if (S0 + max_new > d->n_positions) return fail(VCAP_E_UNSUPPORTED, "context exceeds n_positions");
    r.max_S0 = std::max(r.max_S0, S0);
    r.min_S0 = b == 0 ? S0 : std::min(r.min_S0, S0);
    M += (long)S0 * rep;
    if (M > kMaxDecodeRows) return fail(VCAP_E_UNSUPPORTED, "sum of (prefix+prompt) rows exceeds vcap_gpt2_max_rows()");
  }
  r.M = (int)M;
  r.nids = offsets[B];
  *out = r;
  return 0;
}

int ragged_ids(const char* name, const vcap_gpt2_desc* d, const vcap_prompts* p, const Ragged& r) {
  if (r.nids && !p->ids) return fail(VCAP_E_ARG, std::string(name) + ": bad arguments");
  return check_prompt_ids(d, p->ids, r.nids);
}

void carve_ragged(Carver& c, const vcap_gpt2_desc* d, Ragged& r) {
  r.tab = (int*)c.take(r.tab_ints() * 4);
  r.hl = (float*)c.take((size_t)r.R * d->n_embd * 4);
}

// Tables + ids to the workspace, on the call's stream and outside any captured graph (like the Philox
// seed): a captured graph bakes in the shape only.  The host block is pageable memory, so the copy has
// left it when hipMemcpyAsync returns; it is kept per thread all the same.
int upload_ragged(const vcap_gpt2_desc* d, const Ragged& r, const int* ids, hipStream_t s) {
  thread_local std::vector<int> host;
  host.assign(r.tab_ints(), 0);
  int* row_seq = host.data();
  int* row_pos = row_seq + r.M;
  int* seq_len = row_pos + r.M;
  int* last_row = seq_len + r.R;
  int* ids_off = last_row + r.R;
  int m = 0;
  for (int q = 0; q < r.R; ++q) {
    const int b = q / r.rep, S0 = d->prefix_len + r.offsets[b + 1] - r.offsets[b];
    for (int i = 0; i < S0; ++i, ++m) {
      row_seq[m] = q;
      row_pos[m] = i;
    }
    seq_len[q] = S0;
    last_row[q] = m - 1;
  }
  for (int b = 0; b < r.B; ++b) ids_off[b] = r.offsets[b];
  for (int i = 0; i < r.nids; ++i) ids_off[r.B + i] = ids[i];
  VCAP_TRY(hipMemcpyAsync(r.tab, host.data(), host.size() * 4, hipMemcpyHostToDevice, s), "ragged tables");
  return 0;
}

// run_layers' extras for the packed prefill and for step `t` (the t-th token after the prefill's)
LayerExtras ragged_prefill_rows(const Ragged& r) {
  LayerExtras x;
  x.row_seq = r.row_seq(); x.row_pos = r.row_pos(); x.seq_len = r.seq_len(); x.min_len = r.min_S0;
  return x;
}
LayerExtras ragged_step_rows(const Ragged& r, int t, LayerExtras x = {}) {
  x.row_seq = nullptr; x.row_pos = r.seq_len(); x.pos_add = t; x.min_len = r.min_S0 + t + 1;
  return x;
}

// What vcap_gpt2_generate / _sample / _beam_search were given: issue_decode and issue_beam launch from
// it and the graph key is made of it.  Greedy: gp.  Sampling: gp + sp.  Beam search: bp + out_len.
struct DecodeCall {
  const vcap_gpt2_desc* d;
  const float* prefix;
  const int* ids;
  int nids, B;
  int* out_ids;
  const vcap_gen_params* gp = nullptr;
  float* logits_out = nullptr;
  const vcap_sample_params* sp = nullptr;
  float* warped_out = nullptr;
  const int* force_ids = nullptr;
  const vcap_beam_params* bp = nullptr;
  int* out_len = nullptr;
  const Ragged* rg = nullptr;   // the _ragged entry points: ids / nids unused
};

// sp != nullptr: sampling mode (HF _sample): the lm_head also stores the processed scores, the
// sample kernel warps them and draws (or takes force_ids), and hands the token to the finalize kernel
int issue_decode(const DecodeCall& c, const DecState& w, hipStream_t s) {
  const vcap_gpt2_desc* d = c.d;
  const vcap_gen_params* gp = c.gp;
  const vcap_sample_params* sp = c.sp;
  const int E = d->n_embd, V = d->vocab, B = c.B;
  const Ragged* rg = c.rg;
  const int P = d->prefix_len, S0 = rg ? rg->max_S0 : P + c.nids, max_new = gp->max_new_tokens;
  const int dt = d->dtype;
  VCAP_TRY(vcap_decode_init_dispatch(w.pt, B, w.maxp, w.finished, w.nbanned, s, w.skc, w.n_skc), "decode_init");
  if (rg)
    VCAP_TRY(vcap_prefill_embed_rows_dispatch(dt, c.prefix, P, rg->ids(), rg->ids_off(), rg->row_seq(), rg->row_pos(),
                                              d->wte, d->wpe, w.h, rg->M, E, 1, s),
             "prefill_embed_rows");
  else
    VCAP_TRY(vcap_prefill_embed_dispatch(dt, c.prefix, P, c.ids, c.nids, d->wte, d->wpe, w.h, B, E, s), "prefill_embed");
  for (int step = 0; step < max_new; ++step) {
    // ragged: every row is a "sequence of one row" whose position comes from the tables
    const int S_new = step == 0 && !rg ? S0 : 1;
    const int past = step == 0 ? (rg ? S0 - 1 : 0) : S0 + step - 1;   // ragged: the largest context - 1
    if (!rg) {
      if (int rc = run_layers(d, w, B * S_new, S_new, past, gp->max_blocks, s)) return rc;
    } else if (step == 0) {
      if (int rc = run_layers(d, w, rg->M, 1, past, gp->max_blocks, s, ragged_prefill_rows(*rg))) return rc;
      // the lm_head reads each sequence's last prefill row from a contiguous copy
      VCAP_TRY(vcap_gather_rows_dispatch(w.h, rg->last_row(), rg->hl, B, E, s), "gather_last_rows");
    } else {
      if (int rc = run_layers(d, w, B, 1, past, gp->max_blocks, s, ragged_step_rows(*rg, step - 1))) return rc;
    }
    int nblk = 0;
    RowsGemmArgs g = logits_args(d, w, B, S_new, max_new, step);
    if (rg && step == 0) g.x = rg->hl;
    g.rep_penalty = gp->repetition_penalty; g.min_new = gp->min_new_tokens; g.eos = gp->eos_token_id;
    // f32 greedy: the bf16 lm_head screens, the finalize rescores the survivors in f32 (exact argmax);
    // requested raw logits or sampling need every f32 score - the f32 lm_head then
    ScreenArgs sc{};
    bool screen = false;
    if (dt == VCAP_DT_F32 && d->lm_head_screen && d->screen_bound > 0.f && !c.logits_out && !sp) {
      RowsGemmArgs gs = g;
      gs.w = d->lm_head_screen; gs.proc_out = w.proc; gs.screen_h = w.sh;
      int tpb = 0;
      const hipError_t e = vcap_lm_head_screen_dispatch(gs, &nblk, &tpb, s);
      if (e == hipSuccess) {
        const float rep = gp->repetition_penalty;
        const float pfac = rep >= 1.f ? rep : 1.f / rep;
        sc = ScreenArgs{w.proc, w.sh, (const float*)d->wte, d->screen_bound * pfac, tpb, rep, gp->min_new_tokens};
        screen = true;
      } else if (e != hipErrorNotSupported) {
        return hip_fail(e, "lm_head_screen");
      }
    }
    if (!screen) {
      g.logits_raw = c.logits_out ? c.logits_out + (size_t)step * B * V : nullptr;
      g.nblk = max_logit_blocks(V, B);
      g.proc_out = sp ? w.proc : nullptr;
      VCAP_TRY(vcap_rows_gemm_dispatch(dt, PRO_LN, EPI_LOGITS, g, &nblk, s), "lm_head");
    }
    if (sp) {
      SampleArgs sa{w.proc, V, V, sp->temperature, sp->top_k, sp->top_p, w.seed, step, c.force_ids, max_new,
                    c.warped_out ? c.warped_out + (size_t)step * B * V : nullptr, V, w.pval, w.pidx,
                    gp->eos_token_id};
      VCAP_TRY(vcap_sample_dispatch(sa, B, s), "sample");
      nblk = 1;
    }
    if (rg)
      VCAP_TRY(vcap_decode_finalize_rows_dispatch(dt, w.pval, w.pidx, nblk, B, step, w.finished, w.hist, max_new,
                                                  w.banned, w.nbanned, gp->no_repeat_ngram_size, gp->eos_token_id,
                                                  gp->pad_token_id, c.out_ids, max_new, d->wte, d->wpe, w.h, E,
                                                  rg->seq_len(), step, d->n_positions, V, s, screen ? &sc : nullptr),
               "finalize_rows");
    else
      VCAP_TRY(vcap_decode_finalize_dispatch(dt, w.pval, w.pidx, nblk, B, step, w.finished, w.hist, max_new, w.banned,
                                             w.nbanned, gp->no_repeat_ngram_size, gp->eos_token_id, gp->pad_token_id,
                                             c.out_ids, max_new, d->wte, d->wpe, w.h, E,
                                             (S0 + step) < d->n_positions ? S0 + step : d->n_positions - 1, V, s,
                                             screen ? &sc : nullptr),
               "finalize");
  }
  return 0;
}

// Everything the captured decode bakes in.  The Philox seed is not part of it (it lives in device
// memory, written outside the graph), so one sampling graph serves every seed.
std::string decode_key(const DecodeCall& c, const void* workspace) {
  GraphKey k(c.bp ? "beam" : "");
  k.put_desc(c.d);
  if (c.bp) k.put(c.bp, sizeof(*c.bp));
  else k.put(c.gp, sizeof(*c.gp));
  k.val(c.prefix);
  if (c.rg) {
    // the ids live in the workspace (uploaded outside the graph): the shape alone is baked in
    k.put("ragged", 6);
    k.put(c.rg->offsets, sizeof(int) * (size_t)(c.B + 1));
  } else {
    k.put(c.ids, sizeof(int) * (size_t)c.nids);
    k.val(c.nids);
  }
  k.val(c.B);
  k.val(c.out_ids);
  if (c.bp) k.val(c.out_len);
  else k.val(c.logits_out);
  k.val(workspace);
  k.put_device();
  if (c.sp) {
    vcap_sample_params ks = *c.sp;
    ks.seed = 0;
    k.put("sample", 6);
    k.val(ks);
    k.val(c.warped_out);
    k.val(c.force_ids);
  }
  return k.k;
}

// The seed upload, then the launch: eager, or the cached graph's replay.
int run_decode_carved(const DecodeCall& c, const DecState& w, void* workspace, hipStream_t s) {
  if (c.sp) {
    // the Philox key goes to device memory outside the graph: one captured graph serves every seed
    VCAP_TRY(hipMemsetD32Async((hipDeviceptr_t)w.seed, (int)(uint32_t)c.sp->seed, 1, s), "seed lo");
    VCAP_TRY(hipMemsetD32Async((hipDeviceptr_t)(w.seed + 1), (int)(uint32_t)(c.sp->seed >> 32), 1, s), "seed hi");
  }
  if (!c.gp->use_graph) return issue_decode(c, w, s);
  return launch_cached(decode_key(c, workspace), s, [&](hipStream_t cs) { return issue_decode(c, w, cs); });
}

// The checked call of vcap_gpt2_generate / vcap_gpt2_sample (`name`): carve, then launch eagerly or
// replay the cached graph.
int run_decode(const char* name, const DecodeCall& c, void* workspace, size_t ws_bytes, hipStream_t s) {
  const int S0 = c.d->prefix_len + c.nids, max_new = c.gp->max_new_tokens;
  if (ws_bytes < vcap_gpt2_workspace_bytes(c.d, c.B, S0, max_new))
    return fail(VCAP_E_WORKSPACE, std::string(name) + ": workspace too small");
  Carver cv(workspace);
  const DecState w = carve_dec(cv, c.d, c.B, S0, max_new);
  return run_decode_carved(c, w, workspace, s);
}

// ... and of the _ragged forms (rg checked by ragged_shape / ragged_ids): the tables follow the decode state
int run_decode_ragged(const char* name, DecodeCall c, Ragged rg, const int* ids, void* workspace, size_t ws_bytes,
                      hipStream_t s) {
  Carver cv(workspace);
  const DecState w = carve_dec(cv, c.d, c.B, rg.max_S0, c.gp->max_new_tokens, rg.M);
  carve_ragged(cv, c.d, rg);
  if (ws_bytes < cv.off) return fail(VCAP_E_WORKSPACE, std::string(name) + ": workspace too small");
  if (int rc = upload_ragged(c.d, rg, ids, s)) return rc;
  c.rg = &rg;
  return run_decode_carved(c, w, workspace, s);
}

// ---- the step path (host-bookkeeping beam search): the decode state plus the reorder's scratch pool
struct StepBufs {
  DecState w;
  void* scratch;   // one layer-stacked K or V pool (the reorder gathers one pool at a time)
};

StepBufs carve_step(Carver& c, const vcap_gpt2_desc* d, int rows, int S0, int max_new) {
  StepBufs b;
  b.w = carve_dec(c, d, rows, S0, max_new);
  b.scratch = c.take(b.w.page_elems * d->n_layer * esize(d->dtype));
  return b;
}

int step_setup(const vcap_gpt2_desc* d, int rows, int S0, int max_new, void* ws, size_t ws_bytes, StepBufs* b) {
  if (int rc = check_gpt2_launch(d)) return rc;
  if (rows <= 0 || rows > kMaxDecodeRows || S0 <= 0 || max_new <= 0 || S0 + max_new > d->n_positions)
    return fail(VCAP_E_ARG, "gpt2 step: bad rows / lengths");
  if (ws_bytes < vcap_gpt2_beam_workspace_bytes(d, rows, S0, max_new))
    return fail(VCAP_E_WORKSPACE, "gpt2 step: workspace too small (vcap_gpt2_beam_workspace_bytes)");
  Carver c(ws);
  *b = carve_step(c, d, rows, S0, max_new);
  return 0;
}

// ---- device beam search
struct BeamBufs {
  DecState w;
  float* logits;
  float* part_max;
  float* part_sum;
  BeamState st;
  int nblk, chunks, anc_ld;
};

// prefill_rows > 0 (ragged prompts): S0 is the longest sequence's, see carve_dec
BeamBufs carve_beam(Carver& c, const vcap_gpt2_desc* d, int B, int nb, int S0, int L, int prefill_rows = 0) {
  BeamBufs b;
  const int R = B * nb;
  b.w = carve_dec(c, d, R, S0, L, prefill_rows);
  b.nblk = max_logit_blocks(d->vocab, R);
  b.chunks = vcap_beam_chunks(d->vocab);
  b.anc_ld = S0 + L;
  b.logits = (float*)c.take((size_t)R * d->vocab * 4);
  b.part_max = (float*)c.take((size_t)R * b.nblk * 4);
  b.part_sum = (float*)c.take((size_t)R * b.nblk * 4);
  BeamState& st = b.st;
  const size_t RL = (size_t)R * L * 4;
  st.run_seq = (int*)c.take(RL);
  st.run_bidx = (int*)c.take(RL);
  st.seqs = (int*)c.take(RL);
  st.beam_idx = (int*)c.take(RL);
  st.run_score = (float*)c.take((size_t)R * 4);
  st.beam_score = (float*)c.take((size_t)R * 4);
  st.fin = (int*)c.take((size_t)R * 4);
  st.unsat = (int*)c.take((size_t)B * 4);
  st.stopped = (int*)c.take(4);
  st.tok_next = (int*)c.take((size_t)R * 4);
  st.anc = (int*)c.take((size_t)R * b.anc_ld * 4);
  st.cand_val = (float*)c.take((size_t)R * b.chunks * 2 * nb * 4);
  st.cand_tok = (int*)c.take((size_t)R * b.chunks * 2 * nb * 4);
  return b;
}

int issue_beam(const DecodeCall& c, const BeamBufs& bb, hipStream_t s) {
  const vcap_gpt2_desc* d = c.d;
  const vcap_beam_params* bp = c.bp;
  const int E = d->n_embd, B = c.B, nb = bp->num_beams, L = bp->max_new_tokens, R = B * nb;
  const Ragged* rg = c.rg;
  const int S0 = rg ? rg->max_S0 : d->prefix_len + c.nids;   // ragged: the longest sequence's
  const DecState& w = bb.w;
  int nblk = bb.nblk;  // log_softmax partials per row the lm_head leaves (<= bb.nblk)
  auto lm_head = [&](int S_new, const float* x = nullptr) -> int {
    RowsGemmArgs g = lm_head_args(d, w, R, S_new);
    if (x) g.x = x;
    g.logits_raw = bb.logits; g.part_val = bb.part_max; g.part_sum = bb.part_sum; g.nblk = bb.nblk;
    g.max_blocks = bp->max_blocks;  // the streamed lm_head's grid (<= one workgroup per CU)
    nblk = bb.nblk;
    VCAP_TRY(vcap_rows_gemm_dispatch(d->dtype, PRO_LN, EPI_LSE, g, &nblk, s), "lm_head_lse");
    return 0;
  };
  VCAP_TRY(vcap_decode_init_dispatch(w.pt, R, w.maxp, w.finished, w.nbanned, s, w.skc, w.n_skc), "decode_init");
  // prefill: every beam row gets its sequence's prompt (HF expands the input to B * num_beams)
  if (rg) {
    // the packed prefill: every beam row's own S0 rows; the lm_head over a copy of each one's last row
    VCAP_TRY(vcap_prefill_embed_rows_dispatch(d->dtype, c.prefix, d->prefix_len, rg->ids(), rg->ids_off(),
                                              rg->row_seq(), rg->row_pos(), d->wte, d->wpe, w.h, rg->M, E, nb, s),
             "prefill_embed_rows");
    if (int rc = run_layers(d, w, rg->M, 1, S0 - 1, 0, s, ragged_prefill_rows(*rg))) return rc;
    VCAP_TRY(vcap_gather_rows_dispatch(w.h, rg->last_row(), rg->hl, R, E, s), "gather_last_rows");
    if (int rc = lm_head(1, rg->hl)) return rc;
  } else {
    VCAP_TRY(vcap_prefill_embed_dispatch(d->dtype, c.prefix, d->prefix_len, c.ids, c.nids, d->wte, d->wpe, w.h, R, E,
                                         s, 0, nb),
             "prefill_embed");
    if (int rc = run_layers(d, w, R * S0, S0, 0, 0, s)) return rc;
    if (int rc = lm_head(S0)) return rc;
  }
  VCAP_TRY(vcap_beam_init_dispatch(bb.st, B, nb, L, S0, bb.anc_ld, bp->eos_token_id, s), "beam_init");
  const LayerExtras anc{bb.st.anc, bb.anc_ld};
  for (int cur = 0; cur < L; ++cur) {
    if (cur > 0) {
      const int pos = S0 + cur - 1;
      if (rg) {
        VCAP_TRY(vcap_embed_tokens_rows_dispatch(d->dtype, bb.st.tok_next, R, d->wte, d->wpe, w.h, E, rg->seq_len(),
                                                 cur - 1, d->n_positions, s),
                 "embed_rows");
        if (int rc = run_layers(d, w, R, 1, pos, bp->max_blocks, s, ragged_step_rows(*rg, cur - 1, anc))) return rc;
      } else {
        VCAP_TRY(vcap_embed_tokens_dispatch(d->dtype, bb.st.tok_next, R, d->wte, d->wpe, w.h, E, pos, s), "embed");
        if (int rc = run_layers(d, w, R, 1, pos, bp->max_blocks, s, anc)) return rc;
      }
      if (int rc = lm_head(1)) return rc;
    }
    VCAP_TRY(vcap_beam_cand_dispatch(bb.st, bb.logits, bb.part_max, bb.part_sum, nblk, R, d->vocab, nb, L, cur,
                                     bp->repetition_penalty, bp->no_repeat_ngram_size, bp->min_new_tokens,
                                     bp->eos_token_id, bb.chunks, s),
             "beam_cand");
    VCAP_TRY(vcap_beam_select_dispatch(bb.st, B, nb, L, d->vocab, bb.chunks, cur, bp->eos_token_id,
                                       bp->length_penalty, S0, bb.anc_ld, s, rg ? rg->seq_len() : nullptr),
             "beam_select");
  }
  VCAP_TRY(vcap_beam_output_dispatch(bb.st, B, nb, L, c.out_ids, c.out_len, s), "beam_output");
  return 0;
}

// ---- teacher-forced scoring: the decode state (the paged cache is scratch here) for B sequences of S
// positions, then the all-rows lm_head's operand and partials
struct ScoreBufs {
  DecState w;
  void* xn;        // [B*S][E] ln_f rows, decoder dtype
  float* pmax;     // [B*S][nparts]
  float* psum;
  float* tlogit;   // [B*S]
  float* logprob;  // [B*S]
  int nparts;
};

ScoreBufs carve_score(Carver& c, const vcap_gpt2_desc* d, int B, int S) {
  ScoreBufs b;
  b.w = carve_dec(c, d, B, S, 1);
  const size_t M = (size_t)B * S;
  b.nparts = vcap_score_parts(d->vocab);
  b.xn = c.take(M * d->n_embd * esize(d->dtype));
  b.pmax = (float*)c.take(M * b.nparts * 4);
  b.psum = (float*)c.take(M * b.nparts * 4);
  b.tlogit = (float*)c.take(M * 4);
  b.logprob = (float*)c.take(M * 4);
  return b;
}

}  // namespace

int vcap_gpt2_check_desc(const vcap_gpt2_desc* d, bool launch) { return launch ? check_gpt2_launch(d) : check_gpt2(d); }

// vcap_gpt2_score's schedule (arguments checked by the caller; workspace of vcap_gpt2_score_workspace_bytes).
// snap / out: the backward's residual-stream snapshots (LayerExtras.snap) and the buffers it reads afterwards;
// tail: the operand snapshots of the unfrozen layers (LayerExtras.tail), the tail call only.
int vcap_score_forward(const vcap_gpt2_desc* d, const float* embeds, int B, int S, const uint8_t* key_mask,
                       const int* targets, float* logits_out, float* logprob_out, float* loss_out, void* workspace,
                       float* snap, hipStream_t s, ScoreForward* out, const ScoreTailSnap* tail) {
  Carver c(workspace);
  const ScoreBufs b = carve_score(c, d, B, S);
  const DecState& w = b.w;
  const int M = B * S, E = d->n_embd;
  VCAP_TRY(vcap_decode_init_dispatch(w.pt, B, w.maxp, w.finished, w.nbanned, s, w.skc, w.n_skc), "decode_init");
  // the prefill-embedding kernel with every position taken from `embeds`: h = embeds + wpe[0..S)
  VCAP_TRY(vcap_prefill_embed_dispatch(d->dtype, embeds, S, nullptr, 0, d->wte, d->wpe, w.h, B, E, s), "embed_inputs");
  LayerExtras x{nullptr, 0, key_mask, S};
  x.snap = snap;
  x.tail = tail;
  if (int rc = run_layers(d, w, M, S, 0, 0, s, x)) return rc;
  VCAP_TRY(vcap_layernorm_dispatch(d->dtype, w.h, E, b.xn, E, d->lnf_g, d->lnf_b, M, E, d->ln_eps, s), "ln_f");
  ScoreLmArgs a{b.xn, d->wte, M, d->vocab, E, targets, logits_out, b.pmax, b.psum, b.tlogit, b.nparts};
  VCAP_TRY(vcap_score_lm_dispatch(d->dtype, a, s), "score_lm_head");
  if (targets)
    VCAP_TRY(vcap_score_combine_dispatch(a, key_mask, S, b.logprob, logprob_out, loss_out, s), "score_combine");
  if (out) *out = ScoreForward{b.pmax, b.psum, b.nparts};
  return 0;
}

// =====================================================================================================
extern "C" {

int vcap_gpt2_max_rows(void) { return kMaxDecodeRows; }

size_t vcap_rows_packed_bytes(int dtype, int N, int K) {
  if (dtype != VCAP_DT_F32 && dtype != VCAP_DT_BF16) return 0;
  if (N <= 0 || K <= 0 || K % (dtype == VCAP_DT_BF16 ? 32 : 16)) return 0;
  return vcap_rows_packed_size(dtype, N, K);
}

int vcap_rows_pack(int dtype, const void* w, int64_t ldw, int N, int K, void* packed, void* stream) {
  if (dtype != VCAP_DT_F32 && dtype != VCAP_DT_BF16) return fail(VCAP_E_ARG, "rows_pack dtype");
  if (!w || !packed || ldw < K) return fail(VCAP_E_ARG, "rows_pack: null pointer or ldw < K");
  VCAP_TRY(vcap_rows_pack_dispatch(dtype, w, (long)ldw, N, K, packed, (hipStream_t)stream),
           "rows_pack (K % 32/16, 16-byte aligned rows and pointers)");
  return 0;
}

int vcap_decode_attention(int dtype, const void* q, const void* k_pool, const void* v_pool, const int* page_table,
                          int maxp, void* out, int M, int heads, int S_new, int past, void* stream) {
  if (!q || !k_pool || !v_pool || !out || M <= 0 || heads <= 0 || S_new <= 0 || past < 0 || maxp <= 0 ||
      M % S_new)
    return fail(VCAP_E_ARG, "vcap_decode_attention: bad arguments");
  if (dtype != VCAP_DT_F32 && dtype != VCAP_DT_BF16) return fail(VCAP_E_ARG, "vcap_decode_attention: dtype");
  if (past + S_new > 16 * maxp) return fail(VCAP_E_ARG, "vcap_decode_attention: context exceeds the page table");
  if (!page_table && (dtype != VCAP_DT_BF16 || past + S_new > 64))
    return fail(VCAP_E_UNSUPPORTED, "vcap_decode_attention: a NULL page table needs bf16 and context <= 64");
  DecodeKeys keys;
  keys.page_table = page_table;
  VCAP_TRY(vcap_decode_attention_dispatch(dtype, q, k_pool, v_pool, keys, maxp, out, M, heads, S_new, past,
                                          (hipStream_t)stream),
           "vcap_decode_attention");
  return 0;
}

size_t vcap_gpt2_workspace_bytes(const vcap_gpt2_desc* d, int B, int S0, int max_new_tokens) {
  return check_gpt2(d) ? 0 : carved_bytes([&](Carver& c) { carve_dec(c, d, B, S0, max_new_tokens); });
}

int vcap_gpt2_generate(const vcap_gpt2_desc* d, const vcap_gen_params* gp, const float* prefix, const int* prompt_ids,
                       int prompt_len, int B, int* out_ids, float* logits_out, void* workspace, size_t ws_bytes,
                       void* stream) {
  const char* name = "vcap_gpt2_generate";
  if (int rc = check_gpt2_launch(d)) return rc;
  if (!gp || !out_ids) return fail(VCAP_E_ARG, "vcap_gpt2_generate: bad arguments");
  if (int rc = check_prompt_args(name, prefix, prompt_ids, prompt_len, B)) return rc;
  if (gp->max_new_tokens <= 0) return fail(VCAP_E_ARG, "max_new_tokens must be > 0");
  if (gp->max_new_tokens > 64)
    return fail(VCAP_E_UNSUPPORTED, "max_new_tokens > 64 (the lm_head stages the processors' history in LDS)");
  if (int rc = check_prompt_rows(d, prompt_ids, prompt_len, B, gp->max_new_tokens)) return rc;
  DecodeCall c{d, prefix, prompt_ids, prompt_len, B, out_ids, gp, logits_out};
  return run_decode(name, c, workspace, ws_bytes, (hipStream_t)stream);
}

int vcap_gpt2_sample(const vcap_gpt2_desc* d, const vcap_gen_params* gp, const vcap_sample_params* sp,
                     const float* prefix, const int* prompt_ids, int prompt_len, int B, int* out_ids,
                     float* logits_out, float* warped_out, const int* force_ids, void* workspace, size_t ws_bytes,
                     void* stream) {
  const char* name = "vcap_gpt2_sample";
  if (int rc = check_gpt2_launch(d)) return rc;
  // no context row at all (no prefix, no prompt) is an argument error here; it used to launch on zero rows
  if (!gp || !sp || !out_ids || d->prefix_len + prompt_len <= 0)
    return fail(VCAP_E_ARG, "vcap_gpt2_sample: bad arguments");
  if (int rc = check_prompt_args(name, prefix, prompt_ids, prompt_len, B)) return rc;
  if (!(sp->temperature > 0.f) || !(sp->top_p > 0.0) || sp->top_p > 1.0 || sp->top_k < 1)
    return fail(VCAP_E_ARG, "vcap_gpt2_sample: needs temperature > 0, 0 < top_p <= 1, top_k >= 1");
  if (sp->top_k > vcap_sample_max_top_k() || d->vocab > 50 * 1024)
    return fail(VCAP_E_UNSUPPORTED, "vcap_gpt2_sample: top_k <= 128 and vocab <= 51200");
  if (gp->max_new_tokens <= 0 || gp->max_new_tokens > 64)
    return fail(VCAP_E_UNSUPPORTED, "max_new_tokens must be in 1..64");
  if (int rc = check_prompt_rows(d, prompt_ids, prompt_len, B, gp->max_new_tokens)) return rc;
  DecodeCall c{d, prefix, prompt_ids, prompt_len, B, out_ids, gp, logits_out, sp, warped_out, force_ids};
  return run_decode(name, c, workspace, ws_bytes, (hipStream_t)stream);
}

size_t vcap_gpt2_ragged_workspace_bytes(const vcap_gpt2_desc* d, const int* offsets, int B, int max_new_tokens) {
  Ragged rg;
  if (check_gpt2(d) || max_new_tokens <= 0 || max_new_tokens > 64 ||
      ragged_shape("vcap_gpt2_ragged_workspace_bytes", d, offsets, B, max_new_tokens, 1, VCAP_E_UNSUPPORTED, &rg))
    return 0;
  return carved_bytes([&](Carver& c) {
    carve_dec(c, d, B, rg.max_S0, max_new_tokens, rg.M);
    carve_ragged(c, d, rg);
  });
}

int vcap_gpt2_generate_ragged(const vcap_gpt2_desc* d, const vcap_gen_params* gp, const float* prefix,
                              const vcap_prompts* prompts, int B, int* out_ids, float* logits_out, void* workspace,
                              size_t ws_bytes, void* stream) {
  const char* name = "vcap_gpt2_generate_ragged";
  if (int rc = check_gpt2_launch(d)) return rc;
  if (!gp || !out_ids || !prefix || !prompts) return fail(VCAP_E_ARG, std::string(name) + ": bad arguments");
  if (gp->max_new_tokens <= 0) return fail(VCAP_E_ARG, "max_new_tokens must be > 0");
  if (gp->max_new_tokens > 64)
    return fail(VCAP_E_UNSUPPORTED, "max_new_tokens > 64 (the lm_head stages the processors' history in LDS)");
  Ragged rg;
  if (int rc = ragged_shape(name, d, prompts->offsets, B, gp->max_new_tokens, 1, VCAP_E_UNSUPPORTED, &rg)) return rc;
  if (int rc = ragged_ids(name, d, prompts, rg)) return rc;
  DecodeCall c{d, prefix, nullptr, 0, B, out_ids, gp, logits_out};
  return run_decode_ragged(name, c, rg, prompts->ids, workspace, ws_bytes, (hipStream_t)stream);
}

int vcap_gpt2_sample_ragged(const vcap_gpt2_desc* d, const vcap_gen_params* gp, const vcap_sample_params* sp,
                            const float* prefix, const vcap_prompts* prompts, int B, int* out_ids, float* logits_out,
                            float* warped_out, const int* force_ids, void* workspace, size_t ws_bytes, void* stream) {
  const char* name = "vcap_gpt2_sample_ragged";
  if (int rc = check_gpt2_launch(d)) return rc;
  if (!gp || !sp || !out_ids || !prefix || !prompts) return fail(VCAP_E_ARG, std::string(name) + ": bad arguments");
  if (!(sp->temperature > 0.f) || !(sp->top_p > 0.0) || sp->top_p > 1.0 || sp->top_k < 1)
    return fail(VCAP_E_ARG, std::string(name) + ": needs temperature > 0, 0 < top_p <= 1, top_k >= 1");
  if (sp->top_k > vcap_sample_max_top_k() || d->vocab > 50 * 1024)
    return fail(VCAP_E_UNSUPPORTED, std::string(name) + ": top_k <= 128 and vocab <= 51200");
  if (gp->max_new_tokens <= 0 || gp->max_new_tokens > 64)
    return fail(VCAP_E_UNSUPPORTED, "max_new_tokens must be in 1..64");
  Ragged rg;
  if (int rc = ragged_shape(name, d, prompts->offsets, B, gp->max_new_tokens, 1, VCAP_E_ARG, &rg)) return rc;
  if (int rc = ragged_ids(name, d, prompts, rg)) return rc;
  DecodeCall c{d, prefix, nullptr, 0, B, out_ids, gp, logits_out, sp, warped_out, force_ids};
  return run_decode_ragged(name, c, rg, prompts->ids, workspace, ws_bytes, (hipStream_t)stream);
}

size_t vcap_gpt2_beam_workspace_bytes(const vcap_gpt2_desc* d, int rows, int S0, int max_new_tokens) {
  return check_gpt2(d) ? 0 : carved_bytes([&](Carver& c) { carve_step(c, d, rows, S0, max_new_tokens); });
}

int vcap_gpt2_prefill(const vcap_gpt2_desc* d, const float* prefix, const int* prompt_ids, int prompt_len, int B,
                      int rows, int max_new_tokens, float* logits_out, void* workspace, size_t ws_bytes,
                      void* stream) {
  const int S0 = d ? d->prefix_len + prompt_len : 0;
  if (!logits_out || B > rows) return fail(VCAP_E_ARG, "vcap_gpt2_prefill: bad arguments");
  if (int rc = check_prompt_args("vcap_gpt2_prefill", prefix, prompt_ids, prompt_len, B)) return rc;
  if (B * S0 > kMaxDecodeRows) return fail(VCAP_E_UNSUPPORTED, "B*(prefix+prompt) exceeds vcap_gpt2_max_rows()");
  StepBufs b;
  if (int rc = step_setup(d, rows, S0, max_new_tokens, workspace, ws_bytes, &b)) return rc;
  if (int rc = check_prompt_ids(d, prompt_ids, prompt_len)) return rc;
  const DecState& w = b.w;
  hipStream_t s = (hipStream_t)stream;
  VCAP_TRY(vcap_decode_init_dispatch(w.pt, rows, w.maxp, w.finished, w.nbanned, s, w.skc, w.n_skc), "decode_init");
  VCAP_TRY(vcap_prefill_embed_dispatch(d->dtype, prefix, d->prefix_len, prompt_ids, prompt_len, d->wte, d->wpe, w.h, B,
                                       d->n_embd, s),
           "prefill_embed");
  return run_raw_forward(d, w, B, S0, 0, logits_out, s);
}

int vcap_gpt2_step(const vcap_gpt2_desc* d, const int* tokens, int rows, int S0, int max_new_tokens, int pos,
                   float* logits_out, void* workspace, size_t ws_bytes, void* stream) {
  if (!tokens || !logits_out || pos < S0 || pos >= S0 + max_new_tokens)
    return fail(VCAP_E_ARG, "vcap_gpt2_step: bad arguments (S0 <= pos < S0 + max_new_tokens)");
  StepBufs b;
  if (int rc = step_setup(d, rows, S0, max_new_tokens, workspace, ws_bytes, &b)) return rc;
  hipStream_t s = (hipStream_t)stream;
  VCAP_TRY(vcap_embed_tokens_dispatch(d->dtype, tokens, rows, d->wte, d->wpe, b.w.h, d->n_embd, pos, s), "embed_tokens");
  return run_raw_forward(d, b.w, rows, 1, pos, logits_out, s);
}

int vcap_gpt2_forward_embeds(const vcap_gpt2_desc* d, const float* embeds, int rows, int n_tok, int past_len, int S0,
                             int max_new_tokens, float* logits_out, void* workspace, size_t ws_bytes, void* stream) {
  if (!embeds || !logits_out || rows <= 0) return fail(VCAP_E_ARG, "vcap_gpt2_forward_embeds: bad arguments");
  if (past_len == 0 ? n_tok != S0 : (n_tok != 1 || past_len < S0 || past_len >= S0 + max_new_tokens))
    return fail(VCAP_E_ARG, "vcap_gpt2_forward_embeds: prefill needs n_tok == S0; a step one token at "
                            "S0 <= past_len < S0 + max_new_tokens");
  if (past_len == 0 && rows * S0 > kMaxDecodeRows)
    return fail(VCAP_E_UNSUPPORTED, "rows*S0 exceeds vcap_gpt2_max_rows() at prefill");
  StepBufs b;
  if (int rc = step_setup(d, rows, S0, max_new_tokens, workspace, ws_bytes, &b)) return rc;
  const DecState& w = b.w;
  hipStream_t s = (hipStream_t)stream;
  if (past_len == 0) VCAP_TRY(vcap_decode_init_dispatch(w.pt, rows, w.maxp, w.finished, w.nbanned, s, w.skc, w.n_skc), "decode_init");
  // the prefill-embedding kernel with every position taken from `embeds` (P = n_tok, no prompt ids)
  VCAP_TRY(vcap_prefill_embed_dispatch(d->dtype, embeds, n_tok, nullptr, 0, d->wte, d->wpe, w.h, rows, d->n_embd, s,
                                       past_len),
           "embed_inputs");
  return run_raw_forward(d, w, rows, n_tok, past_len, logits_out, s);
}

int vcap_gpt2_reorder(const vcap_gpt2_desc* d, const int* src_rows, int rows, int S0, int max_new_tokens, int length,
                      void* workspace, size_t ws_bytes, void* stream) {
  if (!src_rows || length <= 0) return fail(VCAP_E_ARG, "vcap_gpt2_reorder: bad arguments");
  StepBufs b;
  if (int rc = step_setup(d, rows, S0, max_new_tokens, workspace, ws_bytes, &b)) return rc;
  const DecState& w = b.w;
  hipStream_t s = (hipStream_t)stream;
  const size_t bytes = w.page_elems * d->n_layer * esize(d->dtype);
  for (void* pool : {w.kc, w.vc}) {
    VCAP_TRY(vcap_kv_gather_dispatch(d->dtype, pool, b.scratch, src_rows, rows, w.maxp, d->n_head, length,
                                     (long)w.page_elems, d->n_layer, s),
             "kv_gather");
    VCAP_TRY(hipMemcpyAsync(pool, b.scratch, bytes, hipMemcpyDeviceToDevice, s), "kv copy-back");
  }
  return 0;
}

size_t vcap_gpt2_score_workspace_bytes(const vcap_gpt2_desc* d, int B, int S) {
  if (check_gpt2(d) || B <= 0 || S <= 0 || d->vocab <= 0) return 0;
  return carved_bytes([&](Carver& c) { carve_score(c, d, B, S); });
}

int vcap_gpt2_score(const vcap_gpt2_desc* d, const float* embeds, int B, int S, const uint8_t* key_mask,
                    const int* targets, float* logits_out, float* logprob_out, float* loss_out, void* workspace,
                    size_t ws_bytes, void* stream) {
  if (int rc = check_gpt2_launch(d)) return rc;
  if (!embeds || B <= 0 || S <= 0 || !workspace) return fail(VCAP_E_ARG, "vcap_gpt2_score: bad arguments");
  if (!logits_out && !targets) return fail(VCAP_E_ARG, "vcap_gpt2_score: neither logits_out nor targets given");
  if ((logprob_out || loss_out) && !targets)
    return fail(VCAP_E_ARG, "vcap_gpt2_score: logprob_out / loss_out need targets");
  if ((long)B * S > kMaxDecodeRows) return fail(VCAP_E_UNSUPPORTED, "B*S exceeds vcap_gpt2_max_rows()");
  if (S > d->n_positions) return fail(VCAP_E_UNSUPPORTED, "S exceeds n_positions");
  if (ws_bytes < vcap_gpt2_score_workspace_bytes(d, B, S))
    return fail(VCAP_E_WORKSPACE, "vcap_gpt2_score: workspace too small (vcap_gpt2_score_workspace_bytes)");
  return vcap_score_forward(d, embeds, B, S, key_mask, targets, logits_out, logprob_out, loss_out, workspace, nullptr,
                            (hipStream_t)stream, nullptr);
}

size_t vcap_gpt2_beam_search_workspace_bytes(const vcap_gpt2_desc* d, int B, int num_beams, int S0,
                                             int max_new_tokens) {
  if (check_gpt2(d) || B <= 0 || num_beams <= 0) return 0;
  return carved_bytes([&](Carver& c) { carve_beam(c, d, B, num_beams, S0, max_new_tokens); });
}

int vcap_gpt2_beam_search(const vcap_gpt2_desc* d, const vcap_beam_params* bp, const float* prefix,
                          const int* prompt_ids, int prompt_len, int B, int* out_ids, int* out_len, void* workspace,
                          size_t ws_bytes, void* stream) {
  if (int rc = check_gpt2_launch(d)) return rc;
  if (!bp || !out_ids || !out_len) return fail(VCAP_E_ARG, "vcap_gpt2_beam_search: bad arguments");
  if (int rc = check_prompt_args("vcap_gpt2_beam_search", prefix, prompt_ids, prompt_len, B)) return rc;
  const int nb = bp->num_beams, L = bp->max_new_tokens, S0 = d->prefix_len + prompt_len;
  if (nb < 2 || nb > 8 || B > 8 || L <= 0 || L > 64 || S0 + L > 128 || S0 + L > d->n_positions)
    return fail(VCAP_E_UNSUPPORTED, "vcap_gpt2_beam_search: needs 2 <= num_beams <= 8, B <= 8, max_new <= 64, "
                                    "prefix + prompt + max_new <= 128");
  if (S0 <= 0 || B * nb * S0 > kMaxDecodeRows) return fail(VCAP_E_UNSUPPORTED, "B*num_beams*(prefix+prompt) exceeds max rows");
  if (bp->early_stopping != 0) return fail(VCAP_E_UNSUPPORTED, "only early_stopping=False (the reference's presets)");
  if (bp->max_blocks < 0) return fail(VCAP_E_ARG, "vcap_gpt2_beam_search: max_blocks < 0");
  if (nb * vcap_beam_chunks(d->vocab) * 2 * nb > 20 * 64)
    return fail(VCAP_E_UNSUPPORTED, "num_beams too large for the vocabulary (candidate registers)");
  if (int rc = check_prompt_ids(d, prompt_ids, prompt_len)) return rc;
  if (ws_bytes < vcap_gpt2_beam_search_workspace_bytes(d, B, nb, S0, L))
    return fail(VCAP_E_WORKSPACE, "vcap_gpt2_beam_search: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  Carver cv(workspace);
  const BeamBufs bb = carve_beam(cv, d, B, nb, S0, L);
  DecodeCall c{d, prefix, prompt_ids, prompt_len, B, out_ids};
  c.bp = bp;
  c.out_len = out_len;
  if (!bp->use_graph) return issue_beam(c, bb, s);
  return launch_cached(decode_key(c, workspace), s, [&](hipStream_t cs) { return issue_beam(c, bb, cs); });
}

// the ragged search's limits beyond ragged_shape's (the uniform search's, with the longest sequence's S0)
static int check_beam_ragged(const vcap_gpt2_desc* d, int B, int nb, int L, const Ragged& rg) {
  if (nb < 2 || nb > 8 || B > 8 || L <= 0 || L > 64 || rg.max_S0 + L > 128)
    return fail(VCAP_E_UNSUPPORTED, "vcap_gpt2_beam_search_ragged: needs 2 <= num_beams <= 8, B <= 8, max_new <= 64, "
                                    "longest prefix + prompt + max_new <= 128");
  if (nb * vcap_beam_chunks(d->vocab) * 2 * nb > 20 * 64)
    return fail(VCAP_E_UNSUPPORTED, "num_beams too large for the vocabulary (candidate registers)");
  return 0;
}

size_t vcap_gpt2_beam_search_ragged_workspace_bytes(const vcap_gpt2_desc* d, const int* offsets, int B, int num_beams,
                                                    int max_new_tokens) {
  const char* name = "vcap_gpt2_beam_search_ragged_workspace_bytes";
  Ragged rg;
  if (check_gpt2(d) || num_beams < 2 || num_beams > 8 || max_new_tokens <= 0 || max_new_tokens > 64 ||
      ragged_shape(name, d, offsets, B, max_new_tokens, num_beams, VCAP_E_UNSUPPORTED, &rg) ||
      check_beam_ragged(d, B, num_beams, max_new_tokens, rg))
    return 0;
  return carved_bytes([&](Carver& c) {
    carve_beam(c, d, B, num_beams, rg.max_S0, max_new_tokens, rg.M);
    carve_ragged(c, d, rg);
  });
}

int vcap_gpt2_beam_search_ragged(const vcap_gpt2_desc* d, const vcap_beam_params* bp, const float* prefix,
                                 const vcap_prompts* prompts, int B, int* out_ids, int* out_len, void* workspace,
                                 size_t ws_bytes, void* stream) {
  const char* name = "vcap_gpt2_beam_search_ragged";
  if (int rc = check_gpt2_launch(d)) return rc;
  if (!bp || !out_ids || !out_len || !prefix || !prompts) return fail(VCAP_E_ARG, std::string(name) + ": bad arguments");
  const int nb = bp->num_beams, L = bp->max_new_tokens;
  if (nb < 2 || nb > 8 || B > 8 || L <= 0 || L > 64)
    return fail(VCAP_E_UNSUPPORTED, std::string(name) + ": needs 2 <= num_beams <= 8, B <= 8, max_new <= 64");
  Ragged rg;
  if (int rc = ragged_shape(name, d, prompts->offsets, B, L, nb, VCAP_E_UNSUPPORTED, &rg)) return rc;
  if (int rc = check_beam_ragged(d, B, nb, L, rg)) return rc;
  if (bp->early_stopping != 0) return fail(VCAP_E_UNSUPPORTED, "only early_stopping=False (the reference's presets)");
  if (bp->max_blocks < 0) return fail(VCAP_E_ARG, std::string(name) + ": max_blocks < 0");
  if (int rc = ragged_ids(name, d, prompts, rg)) return rc;
  hipStream_t s = (hipStream_t)stream;
  Carver cv(workspace);
  const BeamBufs bb = carve_beam(cv, d, B, nb, rg.max_S0, L, rg.M);
  carve_ragged(cv, d, rg);
  if (ws_bytes < cv.off) return fail(VCAP_E_WORKSPACE, std::string(name) + ": workspace too small");
  if (int rc = upload_ragged(d, rg, prompts->ids, s)) return rc;
  DecodeCall c{d, prefix, nullptr, 0, B, out_ids};
  c.bp = bp;
  c.out_len = out_len;
  c.rg = &rg;
  if (!bp->use_graph) return issue_beam(c, bb, s);
  return launch_cached(decode_key(c, workspace), s, [&](hipStream_t cs) { return issue_beam(c, bb, cs); });
}

}  // extern "C"
