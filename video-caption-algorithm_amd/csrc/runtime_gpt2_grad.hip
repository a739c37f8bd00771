// vcap_gpt2_score_backward (include/vcap.h): the gradient of the teacher-forced target log-probs with
// respect to inputs_embeds.  The forward is vcap_gpt2_score's schedule (runtime_gpt2.hip
// vcap_score_forward) with the all-rows logits kept and 2 L + 1 copies of the f32 residual stream taken
// between its launches; the backward walks the layers last to first, recomputing each layer's
// activations from its two snapshots with plain GEMMs and holding the residual gradient in f32.
//
// Per layer, g = the gradient at the layer's output (x1 = the stream after the attention c_proj, x0 =
// the layer's input):
//   xn2 = ln_2(x1); u = xn2 . c_fc + b            recompute: the pre-GELU c_fc output
//   dact = g . mlp_c_proj^T; du = dact * gelu'(u); g += dLN2(x1) . (du . c_fc^T)
//   xn1 = ln_1(x0); q | k | v = xn1 . c_attn + b   recompute
//   dO = g . attn_c_proj^T; dq | dk | dv = attention backward; g += dLN1(x0) . (dqkv . c_attn^T)
// Every product is C[m][n] = sum_k A[m][k] W[n][k] on the 128x128 tile kernel (score_backward.hip), its K
// range cut into slabs of a constant width that a second kernel adds in slab order (deterministic, the
// same at every row count): the
// Conv1D [in, out] matrices as stored are the [N][K] operand of the transposed products, their
// Linear-layout copies that of the recompute.  Kernels, rounding points and the exact-zero argument:
// score_backward.hip.
//
// vcap_gpt2_score_backward_tail is the same walk (score_backward_walk) with side outputs: in the layers
// l >= L - n_tail it also emits the 12 parameter gradients, each from operands the walk holds at that point -
//   d mproj_w = act^T . g, d mproj_b = colsum(g)      act = gelu_new(c_fc): the forward's bits, snapshotted
//   d fc_w = xn2^T . du, d fc_b = colsum(du); d ln2_g / d ln2_b from dy = du . c_fc^T and x1's row stats
//   d aproj_w = att^T . g', d aproj_b = colsum(g')    att = the forward's attention output, snapshotted;
//                                                     g' = the residual gradient after the ln_2 backward
//   d attn_w = xn1^T . dqkv, d attn_b = colsum(dqkv); d ln1_g / d ln1_b from dy = dqkv . c_attn^T and x0
// with g / g' as the operand copy the c_proj^T products read (bf16: gt).  Every product is ONE launch of
// vcap_gpt2_dw_kernel (gpt2_weight_grad.hip: all M rows in one workgroup's loop, no slabs), every column sum
// one launch of the text tower's fixed-order kernel.  The forward takes two more copies per unfrozen layer
// (act, att); frozen layers and the two older entry points take none.
#include <algorithm>

#include "runtime_common.h"

namespace {

// K columns per slab of the lm_head backward and of the block products: constants, so a product's split
// depends on the model's shape alone, never on the rows of the call
constexpr int kLmSlabCols = 2048;
constexpr int kBlockSlabCols = 256;

int slabs_of(int K, int cols) { return (K + cols - 1) / cols; }

struct GradBufs {
  void* fwd;       // vcap_gpt2_score's workspace
  float* logits;   // [M][V]
  float* snap;     // [2 L + 1][M][E]
  float* lse;      // [M]
  void* dl;        // [M][Vpad] T
  float* slabs;    // the running product's K slabs: [slabs][M][N]
  float* g;        // [M][E] residual gradient
  float* dy;       // [M][E]
  void* gt;        // [M][E] T (bf16 decoders: g as a GEMM operand)
  void* xn;        // [M][E] T
  float* u;        // [M][4E]
  float* dact;     // [M][4E]
  void* du;        // [M][4E] T
  float* qkv;      // [M][3E]
  float* dO;       // [M][E]
  void* dqkv;      // [M][3E] T
  float* P;        // [B*H][S][S]
  float* dS;
  int nslab;
};

GradBufs carve_grad(Carver& c, const vcap_gpt2_desc* d, const vcap_gpt2_grad_desc* g, int B, int S) {
  const size_t M = (size_t)B * S, E = d->n_embd, es = esize(d->dtype), L = d->n_layer;
  GradBufs b;
  b.fwd = c.take(vcap_gpt2_score_workspace_bytes(d, B, S));
  b.logits = (float*)c.take(M * d->vocab * 4);
  b.snap = (float*)c.take((2 * L + 1) * M * E * 4);
  b.lse = (float*)c.take(M * 4);
  b.dl = c.take(M * g->vocab_pad * es);
  b.nslab = slabs_of(g->vocab_pad, kLmSlabCols);
  // the largest product's slabs: N * slabs(K) floats per row
  const size_t per_row = std::max({(size_t)b.nslab * E, 4 * E * slabs_of((int)E, kBlockSlabCols),
                                   E * slabs_of((int)(4 * E), kBlockSlabCols)});
  b.slabs = (float*)c.take(per_row * M * 4);
  b.g = (float*)c.take(M * E * 4);
  b.dy = (float*)c.take(M * E * 4);
  b.gt = c.take(M * E * es);
  b.xn = c.take(M * E * es);
  b.u = (float*)c.take(M * 4 * E * 4);
  b.dact = (float*)c.take(M * 4 * E * 4);
  b.du = c.take(M * 4 * E * es);
  b.qkv = (float*)c.take(M * 3 * E * 4);
  b.dO = (float*)c.take(M * E * 4);
  b.dqkv = c.take(M * 3 * E * es);
  b.P = (float*)c.take((size_t)B * d->n_head * S * S * 4);
  b.dS = (float*)c.take((size_t)B * d->n_head * S * S * 4);
  return b;
}

int check_grad_desc(const vcap_gpt2_desc* d, const vcap_gpt2_grad_desc* g) {
  if (!g || !g->layers) return fail(VCAP_E_ARG, "gpt2 grad desc is null");
  if (g->dtype != d->dtype || g->n_embd != d->n_embd || g->n_layer != d->n_layer)
    return fail(VCAP_E_ARG, "gpt2 grad desc: dtype / n_embd / n_layer differ from the decoder's");
  if (d->vocab <= 0 || g->vocab_pad != (d->vocab + 127) / 128 * 128)
    return fail(VCAP_E_ARG, "gpt2 grad desc: vocab_pad is not the vocabulary rounded up to 128");
  return 0;
}

int check_grad_pointers(const vcap_gpt2_desc* d, const vcap_gpt2_grad_desc* g) {
  if (!g->wte_t) return fail(VCAP_E_ARG, "gpt2 grad desc: a weight pointer is null");
  for (int l = 0; l < d->n_layer; ++l) {
    const vcap_gpt2_grad_layer& y = g->layers[l];
    if (!y.attn_c || !y.aproj_c || !y.fc_c || !y.mproj_c || !y.attn_l || !y.fc_l)
      return fail(VCAP_E_ARG, "gpt2 grad desc: a weight pointer is null");
  }
  return 0;
}

// C [M, N] = A [M, K] . W [N, K]^T (+ bias; rnd: rounded to bf16 values) through K slabs of kBlockSlabCols
int block_gemm(int dt, const GradBufs& b, const void* A, const void* W, float* C, int M, int N, int K,
               const float* bias, int rnd, hipStream_t s, const char* where) {
  VCAP_TRY(vcap_grad_gemm_dispatch(dt, A, K, W, K, b.slabs, N, M, N, K, kBlockSlabCols, s), where);
  VCAP_TRY(vcap_grad_slab_sum_dispatch(b.slabs, (long)M * N, slabs_of(K, kBlockSlabCols), bias, N, rnd, C, s), where);
  return 0;
}

// the residual gradient as the A operand of a c_proj^T product
const void* grad_operand(int dt, const GradBufs& b, long n, hipStream_t s, hipError_t* e) {
  if (dt == VCAP_DT_F32) {
    *e = hipSuccess;
    return b.g;
  }
  *e = vcap_grad_to_bf16_dispatch(b.g, n, b.gt, s);
  return b.gt;
}

// ---- the tail call: the same walk plus the weight gradients of the last n_tail layers
struct TailBufs {
  void* att;      // [n_tail][M][E] T   the forward's attention outputs
  void* act;      // [n_tail][M][4E] T  the forward's gelu_new(c_fc) outputs
  float* stats;   // [M][2] a LayerNorm backward's (mean, rstd) for its gamma / beta sums
};

TailBufs carve_tail(Carver& c, const vcap_gpt2_desc* d, int B, int S, int n_tail) {
  const size_t M = (size_t)B * S, E = d->n_embd, es = esize(d->dtype);
  TailBufs t;
  t.att = c.take((size_t)n_tail * M * E * es);
  t.act = c.take((size_t)n_tail * M * 4 * E * es);
  t.stats = (float*)c.take(M * 2 * 4);
  return t;
}

int check_param_grads(const vcap_gpt2_desc* d, const vcap_gpt2_param_grads* pg) {
  if (!pg || !pg->layers) return fail(VCAP_E_ARG, "vcap_gpt2_score_backward_tail: param_grads is null");
  if (pg->n_tail < 1 || pg->n_tail > d->n_layer)
    return fail(VCAP_E_ARG, "vcap_gpt2_score_backward_tail: n_tail outside 1 .. n_layer");
  for (int i = 0; i < pg->n_tail; ++i) {
    const vcap_gpt2_param_grads_layer& y = pg->layers[i];
    if (!y.ln1_g || !y.ln1_b || !y.attn_w || !y.attn_b || !y.aproj_w || !y.aproj_b || !y.ln2_g || !y.ln2_b ||
        !y.fc_w || !y.fc_b || !y.mproj_w || !y.mproj_b)
      return fail(VCAP_E_ARG, "vcap_gpt2_score_backward_tail: a gradient pointer is null");
  }
  return 0;
}

// dW [K, N] = X^T . dY and db [N] = the column sum of dY; X [M, K], dY [M, N] in the decoder dtype
int weight_grad(int dt, const void* X, const void* dY, int M, int K, int N, float* dW, float* db, hipStream_t s,
                const char* where) {
  VCAP_TRY(vcap_gpt2_dw_dispatch(dt, X, dY, dW, M, K, N, s), where);
  VCAP_TRY(vcap_colsum_dispatch(dt, dY, M, N, db, s), where);
  return 0;
}

// g += dLN(x) . dy; in an unfrozen layer also dgamma / dbeta from the same dy and the row stats
int ln_backward(const float* x, const float* dy, const float* gamma, float eps, int M, int E, float* g,
                const TailBufs* t, float* dgamma, float* dbeta, hipStream_t s, const char* where) {
  if (!dgamma) {
    VCAP_TRY(vcap_ln_backward_dispatch(x, dy, gamma, eps, M, E, g, s), where);
    return 0;
  }
  VCAP_TRY(vcap_ln_backward_stats_dispatch(x, dy, gamma, eps, M, E, g, t->stats, s), where);
  VCAP_TRY(vcap_ln_colsum_dispatch(dy, x, t->stats, M, E, dgamma, dbeta, s), where);
  return 0;
}

// Everything both entry points check, in vcap_gpt2_score_backward's order; pg: the tail call's struct
int check_call(const char* name, const vcap_gpt2_desc* d, const vcap_gpt2_grad_desc* g, const float* embeds, int B,
               int S, const int* targets, const float* grad_embeds, const void* workspace, size_t ws_bytes,
               const vcap_gpt2_param_grads* pg, bool tail) {
  const std::string who(name);
  if (int rc = vcap_gpt2_check_desc(d, true)) return rc;
  if (int rc = check_grad_desc(d, g)) return rc;
  if (int rc = check_grad_pointers(d, g)) return rc;
  if (!embeds || B <= 0 || S <= 0 || !workspace) return fail(VCAP_E_ARG, who + ": bad arguments");
  if (!targets || !grad_embeds) return fail(VCAP_E_ARG, who + ": targets and grad_embeds are required");
  if (tail)
    if (int rc = check_param_grads(d, pg)) return rc;
  if ((long)B * S > vcap_gpt2_max_rows()) return fail(VCAP_E_UNSUPPORTED, "B*S exceeds vcap_gpt2_max_rows()");
  if (S > d->n_positions) return fail(VCAP_E_UNSUPPORTED, "S exceeds n_positions");
  const size_t need = tail ? vcap_gpt2_score_backward_tail_workspace_bytes(d, g, B, S, pg->n_tail)
                           : vcap_gpt2_score_backward_workspace_bytes(d, g, B, S);
  if (ws_bytes < need)
    return fail(VCAP_E_WORKSPACE, who + ": workspace too small (" + who + "_workspace_bytes)");
  return 0;
}

// The forward and the walk of both entry points (arguments checked).  pg == nullptr: the activation
// gradient alone, every launch vcap_gpt2_score_backward always made.  Otherwise the layers l >= L - n_tail
// also emit their parameter gradients from the operands the walk holds at that point.
int score_backward_walk(const vcap_gpt2_desc* d, const vcap_gpt2_grad_desc* g, const float* embeds, int B, int S,
                        const uint8_t* key_mask, const int* targets, const float* grad_logprob, float* grad_embeds,
                        const vcap_gpt2_param_grads* pg, float* logprob_out, float* loss_out, void* workspace,
                        hipStream_t s) {
  Carver c(workspace);
  const GradBufs b = carve_grad(c, d, g, B, S);
  const int dt = d->dtype, M = B * S, E = d->n_embd, H = d->n_head, L = d->n_layer, V = d->vocab, Vp = g->vocab_pad;
  const int first = pg ? L - pg->n_tail : L;   // the first unfrozen layer
  TailBufs t{};
  if (pg) t = carve_tail(c, d, B, S, pg->n_tail);
  const ScoreTailSnap ts{t.att, t.act, first};
  const long n = (long)M * E;
  const size_t es = esize(dt);
  const int rnd = dt == VCAP_DT_BF16;
  hipError_t e;

  ScoreForward f{};
  if (int rc = vcap_score_forward(d, embeds, B, S, key_mask, targets, b.logits, logprob_out, loss_out, b.fwd, b.snap, s,
                                  &f, pg ? &ts : nullptr))
    return rc;

  // lm_head and ln_f
  VCAP_TRY(vcap_score_dlogit_dispatch(dt, f.pmax, f.psum, f.nparts, b.logits, targets, grad_logprob, M, V, Vp, b.lse,
                                      b.dl, s),
           "score_dlogit");
  VCAP_TRY(vcap_grad_gemm_dispatch(dt, b.dl, Vp, g->wte_t, Vp, b.slabs, E, M, E, Vp, kLmSlabCols, s),
           "lm_head_backward");
  VCAP_TRY(vcap_grad_slab_sum_dispatch(b.slabs, n, b.nslab, nullptr, E, 0, b.dy, s), "lm_head_backward_sum");
  VCAP_TRY(hipMemsetAsync(b.g, 0, (size_t)n * 4, s), "grad_zero");
  VCAP_TRY(vcap_ln_backward_dispatch(b.snap + 2 * (size_t)L * n, b.dy, d->lnf_g, d->ln_eps, M, E, b.g, s),
           "ln_f_backward");

  for (int l = L - 1; l >= 0; --l) {
    const vcap_gpt2_layer& ly = d->layers[l];
    const vcap_gpt2_grad_layer& gy = g->layers[l];
    const vcap_gpt2_param_grads_layer* py = l >= first ? &pg->layers[l - first] : nullptr;
    const float* x0 = b.snap + 2 * (size_t)l * n;
    const float* x1 = x0 + n;
    // mlp
    VCAP_TRY(vcap_layernorm_dispatch(dt, x1, E, b.xn, E, ly.ln2_g, ly.ln2_b, M, E, d->ln_eps, s), "ln_2");
    if (int rc = block_gemm(dt, b, b.xn, gy.fc_l, b.u, M, 4 * E, E, ly.fc_b, 0, s, "c_fc")) return rc;
    const void* ga = grad_operand(dt, b, n, s, &e);
    VCAP_TRY(e, "grad_operand");
    if (py) {
      const char* act = (const char*)t.act + (size_t)(l - first) * 4 * n * es;
      if (int rc = weight_grad(dt, act, ga, M, 4 * E, E, py->mproj_w, py->mproj_b, s, "mlp_c_proj_weight_grad"))
        return rc;
    }
    if (int rc = block_gemm(dt, b, ga, gy.mproj_c, b.dact, M, 4 * E, E, nullptr, 0, s, "mlp_c_proj_backward")) return rc;
    VCAP_TRY(vcap_gelu_backward_dispatch(dt, b.u, b.dact, (long)M * 4 * E, b.du, s), "gelu_backward");
    if (py)
      if (int rc = weight_grad(dt, b.xn, b.du, M, E, 4 * E, py->fc_w, py->fc_b, s, "c_fc_weight_grad")) return rc;
    if (int rc = block_gemm(dt, b, b.du, gy.fc_c, b.dy, M, E, 4 * E, nullptr, 0, s, "c_fc_backward")) return rc;
    if (int rc = ln_backward(x1, b.dy, ly.ln2_g, d->ln_eps, M, E, b.g, &t, py ? py->ln2_g : nullptr,
                             py ? py->ln2_b : nullptr, s, "ln_2_backward"))
      return rc;
    // attention
    VCAP_TRY(vcap_layernorm_dispatch(dt, x0, E, b.xn, E, ly.ln1_g, ly.ln1_b, M, E, d->ln_eps, s), "ln_1");
    if (int rc = block_gemm(dt, b, b.xn, gy.attn_l, b.qkv, M, 3 * E, E, ly.attn_b, rnd, s, "c_attn")) return rc;
    ga = grad_operand(dt, b, n, s, &e);
    VCAP_TRY(e, "grad_operand");
    if (py) {
      const char* att = (const char*)t.att + (size_t)(l - first) * n * es;
      if (int rc = weight_grad(dt, att, ga, M, E, E, py->aproj_w, py->aproj_b, s, "attn_c_proj_weight_grad")) return rc;
    }
    if (int rc = block_gemm(dt, b, ga, gy.aproj_c, b.dO, M, E, E, nullptr, 0, s, "attn_c_proj_backward")) return rc;
    VCAP_TRY(vcap_attn_backward_dispatch(dt, b.qkv, b.dO, key_mask, B, S, H, b.P, b.dS, b.dqkv, s),
             "attention_backward");
    if (py)
      if (int rc = weight_grad(dt, b.xn, b.dqkv, M, E, 3 * E, py->attn_w, py->attn_b, s, "c_attn_weight_grad"))
        return rc;
    if (int rc = block_gemm(dt, b, b.dqkv, gy.attn_c, b.dy, M, E, 3 * E, nullptr, 0, s, "c_attn_backward")) return rc;
    if (int rc = ln_backward(x0, b.dy, ly.ln1_g, d->ln_eps, M, E, b.g, &t, py ? py->ln1_g : nullptr,
                             py ? py->ln1_b : nullptr, s, "ln_1_backward"))
      return rc;
  }
  VCAP_TRY(vcap_grad_finish_dispatch(b.g, key_mask, B, S, E, grad_embeds, s), "grad_finish");
  return 0;
}

}  // namespace

extern "C" {

size_t vcap_gpt2_score_backward_workspace_bytes(const vcap_gpt2_desc* d, const vcap_gpt2_grad_desc* g, int B, int S) {
  if (vcap_gpt2_check_desc(d, false) || check_grad_desc(d, g) || B <= 0 || S <= 0) return 0;
  if ((long)B * S > vcap_gpt2_max_rows() || S > d->n_positions) return 0;
  return carved_bytes([&](Carver& c) { carve_grad(c, d, g, B, S); });
}

int vcap_gpt2_score_backward(const vcap_gpt2_desc* d, const vcap_gpt2_grad_desc* g, const float* embeds, int B, int S,
                             const uint8_t* key_mask, const int* targets, const float* grad_logprob,
                             float* grad_embeds, float* logprob_out, float* loss_out, void* workspace,
                             size_t ws_bytes, void* stream) {
  if (int rc = check_call("vcap_gpt2_score_backward", d, g, embeds, B, S, targets, grad_embeds, workspace, ws_bytes,
                          nullptr, false))
    return rc;
  return score_backward_walk(d, g, embeds, B, S, key_mask, targets, grad_logprob, grad_embeds, nullptr, logprob_out,
                             loss_out, workspace, (hipStream_t)stream);
}

size_t vcap_gpt2_score_backward_tail_workspace_bytes(const vcap_gpt2_desc* d, const vcap_gpt2_grad_desc* g, int B,
                                                     int S, int n_tail) {
  const size_t base = vcap_gpt2_score_backward_workspace_bytes(d, g, B, S);
  if (!base || n_tail < 1 || n_tail > d->n_layer) return 0;
  return base + carved_bytes([&](Carver& c) { carve_tail(c, d, B, S, n_tail); });
}

int vcap_gpt2_score_backward_tail(const vcap_gpt2_desc* d, const vcap_gpt2_grad_desc* g, const float* embeds, int B,
                                  int S, const uint8_t* key_mask, const int* targets, const float* grad_logprob,
                                  float* grad_embeds, const vcap_gpt2_param_grads* param_grads, float* logprob_out,
                                  float* loss_out, void* workspace, size_t ws_bytes, void* stream) {
  if (int rc = check_call("vcap_gpt2_score_backward_tail", d, g, embeds, B, S, targets, grad_embeds, workspace,
                          ws_bytes, param_grads, true))
    return rc;
  return score_backward_walk(d, g, embeds, B, S, key_mask, targets, grad_logprob, grad_embeds, param_grads,
                             logprob_out, loss_out, workspace, (hipStream_t)stream);
}

int vcap_gpt2_weight_grad(int dtype, const void* X, const void* dY, float* dW, int M, int K, int N, void* stream) {
  if (dtype != VCAP_DT_F32 && dtype != VCAP_DT_BF16) return fail(VCAP_E_ARG, "vcap_gpt2_weight_grad: dtype");
  if (!X || !dY || !dW || ((uintptr_t)X & 15) || ((uintptr_t)dY & 15) || ((uintptr_t)dW & 15))
    return fail(VCAP_E_ARG, "vcap_gpt2_weight_grad: null or unaligned pointer");
  if (M < 1 || K < 1 || N < 1) return fail(VCAP_E_ARG, "vcap_gpt2_weight_grad: bad sizes");
  if (M > vcap_gpt2_max_rows()) return fail(VCAP_E_UNSUPPORTED, "M exceeds vcap_gpt2_max_rows()");
  if (K % 64 || N % 128) return fail(VCAP_E_UNSUPPORTED, "vcap_gpt2_weight_grad: K % 64 or N % 128");
  VCAP_TRY(vcap_gpt2_dw_dispatch(dtype, X, dY, dW, M, K, N, (hipStream_t)stream), "gpt2_weight_grad");
  return 0;
}

}  // extern "C"
