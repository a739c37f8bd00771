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
  if (int rc = vcap_gpt2_check_desc(d, true)) return rc;
  if (int rc = check_grad_desc(d, g)) return rc;
  if (int rc = check_grad_pointers(d, g)) return rc;
  if (!embeds || B <= 0 || S <= 0 || !workspace) return fail(VCAP_E_ARG, "vcap_gpt2_score_backward: bad arguments");
  if (!targets || !grad_embeds)
    return fail(VCAP_E_ARG, "vcap_gpt2_score_backward: targets and grad_embeds are required");
  if ((long)B * S > vcap_gpt2_max_rows()) return fail(VCAP_E_UNSUPPORTED, "B*S exceeds vcap_gpt2_max_rows()");
  if (S > d->n_positions) return fail(VCAP_E_UNSUPPORTED, "S exceeds n_positions");
  if (ws_bytes < vcap_gpt2_score_backward_workspace_bytes(d, g, B, S))
    return fail(VCAP_E_WORKSPACE,
                "vcap_gpt2_score_backward: workspace too small (vcap_gpt2_score_backward_workspace_bytes)");
  hipStream_t s = (hipStream_t)stream;
  Carver c(workspace);
  const GradBufs b = carve_grad(c, d, g, B, S);
  const int dt = d->dtype, M = B * S, E = d->n_embd, H = d->n_head, L = d->n_layer, V = d->vocab, Vp = g->vocab_pad;
  const long n = (long)M * E;
  const int rnd = dt == VCAP_DT_BF16;
  hipError_t e;

  ScoreForward f{};
  if (int rc = vcap_score_forward(d, embeds, B, S, key_mask, targets, b.logits, logprob_out, loss_out, b.fwd, b.snap, s,
                                  &f))
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
    const float* x0 = b.snap + 2 * (size_t)l * n;
    const float* x1 = x0 + n;
    // mlp
    VCAP_TRY(vcap_layernorm_dispatch(dt, x1, E, b.xn, E, ly.ln2_g, ly.ln2_b, M, E, d->ln_eps, s), "ln_2");
    if (int rc = block_gemm(dt, b, b.xn, gy.fc_l, b.u, M, 4 * E, E, ly.fc_b, 0, s, "c_fc")) return rc;
    const void* ga = grad_operand(dt, b, n, s, &e);
    VCAP_TRY(e, "grad_operand");
    if (int rc = block_gemm(dt, b, ga, gy.mproj_c, b.dact, M, 4 * E, E, nullptr, 0, s, "mlp_c_proj_backward")) return rc;
    VCAP_TRY(vcap_gelu_backward_dispatch(dt, b.u, b.dact, (long)M * 4 * E, b.du, s), "gelu_backward");
    if (int rc = block_gemm(dt, b, b.du, gy.fc_c, b.dy, M, E, 4 * E, nullptr, 0, s, "c_fc_backward")) return rc;
    VCAP_TRY(vcap_ln_backward_dispatch(x1, b.dy, ly.ln2_g, d->ln_eps, M, E, b.g, s), "ln_2_backward");
    // attention
    VCAP_TRY(vcap_layernorm_dispatch(dt, x0, E, b.xn, E, ly.ln1_g, ly.ln1_b, M, E, d->ln_eps, s), "ln_1");
    if (int rc = block_gemm(dt, b, b.xn, gy.attn_l, b.qkv, M, 3 * E, E, ly.attn_b, rnd, s, "c_attn")) return rc;
    ga = grad_operand(dt, b, n, s, &e);
    VCAP_TRY(e, "grad_operand");
    if (int rc = block_gemm(dt, b, ga, gy.aproj_c, b.dO, M, E, E, nullptr, 0, s, "attn_c_proj_backward")) return rc;
    VCAP_TRY(vcap_attn_backward_dispatch(dt, b.qkv, b.dO, key_mask, B, S, H, b.P, b.dS, b.dqkv, s),
             "attention_backward");
    if (int rc = block_gemm(dt, b, b.dqkv, gy.attn_c, b.dy, M, E, 3 * E, nullptr, 0, s, "c_attn_backward")) return rc;
    VCAP_TRY(vcap_ln_backward_dispatch(x0, b.dy, ly.ln1_g, d->ln_eps, M, E, b.g, s), "ln_1_backward");
  }
  VCAP_TRY(vcap_grad_finish_dispatch(b.g, key_mask, B, S, E, grad_embeds, s), "grad_finish");
  return 0;
}

}  // extern "C"
