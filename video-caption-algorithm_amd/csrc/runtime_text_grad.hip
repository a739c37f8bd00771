// vcap_text_encode_backward (include/vcap.h): the gradient of a scalar of the text tower's unit-norm rows
// with respect to every text-tower parameter.  The forward is vcap_text_encode's schedule (runtime_text.hip
// vcap_text_forward) with each layer's q | k | v, attention output and ReLU output left in buffers of their
// own and four copies of the f32 stream per layer; the backward walks the layers last to first.
//
// Per post-LN layer, g = the gradient at the layer's output x2 = LN2(s2), s2 = x1 + linear2(relu(linear1(x1))),
// x1 = LN1(s1), s1 = x0 + out_proj(attn(in_proj(x0))):
//   ds2 = dLN2(s2) . g                  dgamma2, dbeta2
//   dlinear2: db = colsum(ds2), dW = ds2^T . act, dact = ds2 . W2;  du = dact [act > 0]
//   dlinear1: db = colsum(du),  dW = du^T . x1,   dx1 = du . W1
//   ds1 = dLN1(s1) . (ds2 + dx1)        dgamma1, dbeta1
//   dout_proj: db = colsum(ds1), dW = ds1^T . attn, dO = ds1 . Wo;  dq | dk | dv = attention backward
//   din_proj: db = colsum(dqkv), dW = dqkv^T . x0,  dx0 = dqkv . Win;  the layer's input gradient = ds1 + dx0
// The last sum is taken by its consumer: the LayerNorm backward of the layer below, or the embedding rows.
// Every product is C[m][n] = sum_k A[m][k] W[n][k] on vcap_grad_gemm_kernel, its K range cut into slabs of a
// constant width that vcap_grad_slab_sum_kernel adds in slab order.  Kernels, summation orders and the
// exact-zero argument: text_backward.hip.
#include <algorithm>

#include "runtime_common.h"

namespace {

constexpr int kDxSlabCols = 256;   // K columns per slab of the dx = dy . W products (K = E, F or 3E)
constexpr int kDwSlabRows = 128;   // rows (K = Mpad) per slab of the dW = dY^T . X products

int slabs_of(int K, int cols) { return (K + cols - 1) / cols; }
int mpad_of(int dt, int M) {
  const int bk = vcap_grad_bk(dt);
  return (M + bk - 1) / bk * bk;
}

struct TextGradBufs {
  void* fwd;       // vcap_text_encode's workspace; its first M * E floats end as the encoder output
  TextSnap snap;
  float* dy;       // [B][P]
  float* pooled;   // [B][E]
  float* g;        // [M][E] gradient at a layer's output / ds1
  float* ds;       // [M][E] ds2, then ds2 + dx1
  float* d2;       // [M][E] a dx product
  float* dO;       // [M][E]
  float* stats;    // [M][2]
  float* wide;     // [M][max(F, 3E)] f32: dact / du, dq | dk | dv
  void* opr;       // [M][max(F, 3E)] T: a row gradient as a bf16 operand
  void* tA;        // [max(F, 3E)][Mpad] T: dY^T
  void* tB;        // [max(F, E)][Mpad] T: X^T
  float* slabs;    // the running product's K slabs
  float* P;        // [B*H][L][L]
  float* dS;
  int* slot;       // [M]
};

TextGradBufs carve_text_grad(Carver& c, const vcap_text_desc* d, int B, int L) {
  const size_t M = (size_t)B * L, E = d->dim, F = d->ffn, es = esize(d->dtype), nl = d->n_layer;
  const size_t W = std::max(F, 3 * E), Mp = mpad_of(d->dtype, (int)M);
  TextGradBufs b;
  b.fwd = c.take(vcap_text_workspace_bytes(d, B, L));
  b.snap.x = (float*)c.take(nl * 4 * M * E * 4);
  b.snap.qkv = (char*)c.take(nl * M * 3 * E * es);
  b.snap.attn = (char*)c.take(nl * M * E * es);
  b.snap.act = (char*)c.take(nl * M * F * es);
  b.dy = (float*)c.take((size_t)B * d->proj_dim * 4);
  b.pooled = (float*)c.take((size_t)B * E * 4);
  b.g = (float*)c.take(M * E * 4);
  b.ds = (float*)c.take(M * E * 4);
  b.d2 = (float*)c.take(M * E * 4);
  b.dO = (float*)c.take(M * E * 4);
  b.stats = (float*)c.take(M * 2 * 4);
  b.wide = (float*)c.take(M * W * 4);
  b.opr = c.take(M * W * es);
  b.tA = c.take(W * Mp * es);
  b.tB = c.take(std::max(F, E) * Mp * es);
  // the largest product's slabs: dx [slabs(K)][M][N], dW [slabs(Mpad)][rows][N]
  const size_t dx = std::max({W * slabs_of((int)E, kDxSlabCols), E * slabs_of((int)W, kDxSlabCols)}) * M;
  const size_t dw = std::max(3 * E * E, E * F) * slabs_of((int)Mp, kDwSlabRows);
  b.slabs = (float*)c.take(std::max(dx, dw) * 4);
  b.P = (float*)c.take((size_t)B * d->n_head * L * L * 4);
  b.dS = (float*)c.take((size_t)B * d->n_head * L * L * 4);
  b.slot = (int*)c.take(M * 4);
  return b;
}

int check_text_grad_desc(const vcap_text_desc* d, const vcap_text_grad_desc* g) {
  if (!g) return fail(VCAP_E_ARG, "text grad desc is null");
  if (g->dtype != d->dtype || g->dim != d->dim || g->ffn != d->ffn || g->n_layer != d->n_layer)
    return fail(VCAP_E_ARG, "text grad desc: dtype / dim / ffn / n_layer differ from the text desc's");
  return 0;
}

struct Ctx {
  int dt, M, Mp;
  const TextGradBufs* b;
  hipStream_t s;
};

// C [M, N] = A [M, K] . Wt [N, K]^T, A an f32 row gradient (rounded to bf16 first in a bf16 tower)
int dx_gemm(const Ctx& c, const float* A, const void* Wt, float* C, int N, int K, const char* where) {
  const void* a = A;
  if (c.dt == VCAP_DT_BF16) {
    VCAP_TRY(vcap_grad_to_bf16_dispatch(A, (long)c.M * K, c.b->opr, c.s), where);
    a = c.b->opr;
  }
  VCAP_TRY(vcap_grad_gemm_dispatch(c.dt, a, K, Wt, K, c.b->slabs, N, c.M, N, K, kDxSlabCols, c.s), where);
  VCAP_TRY(vcap_grad_slab_sum_dispatch(c.b->slabs, (long)c.M * N, slabs_of(K, kDxSlabCols), nullptr, N, 0, C, c.s),
           where);
  return 0;
}

// db [R] = colsum(dY), dW [R, N] = dY^T . X; dY f32 [M, R], X [M, N] f32 (x_f32) or T
int dw_gemm(const Ctx& c, const float* dY, int R, const void* X, int x_f32, int N, float* dW, float* db,
            const char* where) {
  VCAP_TRY(vcap_text_colsum_dispatch(dY, c.M, R, db, c.s), where);
  VCAP_TRY(vcap_text_transpose_dispatch(c.dt, 1, dY, c.M, R, c.Mp, c.b->tA, c.s), where);
  VCAP_TRY(vcap_text_transpose_dispatch(c.dt, x_f32, X, c.M, N, c.Mp, c.b->tB, c.s), where);
  VCAP_TRY(vcap_grad_gemm_dispatch(c.dt, c.b->tA, c.Mp, c.b->tB, c.Mp, c.b->slabs, N, R, N, c.Mp, kDwSlabRows, c.s),
           where);
  VCAP_TRY(vcap_grad_slab_sum_dispatch(c.b->slabs, (long)R * N, slabs_of(c.Mp, kDwSlabRows), nullptr, N, 0, dW, c.s),
           where);
  return 0;
}

}  // namespace

extern "C" {

size_t vcap_text_encode_backward_workspace_bytes(const vcap_text_desc* d, const vcap_text_grad_desc* g, int B, int L) {
  if (vcap_text_limits(d, B, L, "vcap_text_encode_backward_workspace_bytes") || check_text_grad_desc(d, g)) return 0;
  return carved_bytes([&](Carver& c) { carve_text_grad(c, d, B, L); });
}

int vcap_text_encode_backward(const vcap_text_desc* d, const vcap_text_grad_desc* g, const int* ids, int B, int L,
                              const float* grad_out, const vcap_text_param_grads* grads, float* out, void* workspace,
                              size_t ws_bytes, void* stream) {
  if (int rc = vcap_text_limits(d, B, L, "vcap_text_encode_backward")) return rc;
  if (int rc = check_text_grad_desc(d, g)) return rc;
  if (!ids || !out || !workspace || !grad_out || !grads)
    return fail(VCAP_E_ARG, "vcap_text_encode_backward: null pointer");
  if (int rc = vcap_text_check_pointers(d, workspace)) return rc;
  if (d->n_layer > 0 && (!g->layers || !grads->layers))
    return fail(VCAP_E_ARG, "vcap_text_encode_backward: layers pointer is null");
  if (!grads->proj_w || !grads->proj_b || !grads->emb_ids || !grads->emb_rows || !grads->emb_count)
    return fail(VCAP_E_ARG, "vcap_text_encode_backward: a gradient pointer is null");
  for (int l = 0; l < d->n_layer; ++l) {
    const vcap_text_grad_layer& w = g->layers[l];
    const vcap_text_param_grads_layer& y = grads->layers[l];
    if (!w.in_t || !w.out_t || !w.fc1_t || !w.fc2_t)
      return fail(VCAP_E_ARG, "vcap_text_encode_backward: grad desc layer " + std::to_string(l) + " has a null pointer");
    if (!y.in_w || !y.in_b || !y.out_w || !y.out_b || !y.ln1_g || !y.ln1_b || !y.fc1_w || !y.fc1_b || !y.fc2_w ||
        !y.fc2_b || !y.ln2_g || !y.ln2_b)
      return fail(VCAP_E_ARG, "vcap_text_encode_backward: a gradient pointer of layer " + std::to_string(l) + " is null");
    if (((uintptr_t)w.in_t & 15) || ((uintptr_t)w.out_t & 15) || ((uintptr_t)w.fc1_t & 15) || ((uintptr_t)w.fc2_t & 15) ||
        ((uintptr_t)y.in_w & 15) || ((uintptr_t)y.out_w & 15) || ((uintptr_t)y.fc1_w & 15) || ((uintptr_t)y.fc2_w & 15))
      return fail(VCAP_E_UNSUPPORTED, "vcap_text_encode_backward: weight copies and weight gradients must be 16-byte aligned");
  }
  if (ws_bytes < carved_bytes([&](Carver& c) { carve_text_grad(c, d, B, L); }))
    return fail(VCAP_E_WORKSPACE,
                "vcap_text_encode_backward: workspace too small (vcap_text_encode_backward_workspace_bytes)");

  hipStream_t s = (hipStream_t)stream;
  Carver cv(workspace);
  const TextGradBufs b = carve_text_grad(cv, d, B, L);
  const int dt = d->dtype, M = B * L, E = d->dim, F = d->ffn, H = d->n_head, P = d->proj_dim;
  const size_t n = (size_t)M * E, es = esize(dt);
  const Ctx c{dt, M, mpad_of(dt, M), &b, s};

  if (int rc = vcap_text_forward(d, ids, B, L, out, nullptr, b.fwd, &b.snap, s)) return rc;
  const float* hidden = (const float*)b.fwd;
  VCAP_TRY(vcap_text_tail_bwd_dispatch(hidden, ids, d->pad_id, B, L, E, d->proj_w, d->proj_b, P, out, grad_out, b.dy,
                                       b.pooled, b.g, grads->proj_w, grads->proj_b, s),
           "text_tail_backward");
  const float* pending = nullptr;   // a dx still to be added to b.g (module comment)
  for (int l = d->n_layer - 1; l >= 0; --l) {
    const vcap_text_layer& ly = d->layers[l];
    const vcap_text_grad_layer& wt = g->layers[l];
    const vcap_text_param_grads_layer& y = grads->layers[l];
    const float* x0 = b.snap.x + (size_t)l * 4 * n;
    const float *s1 = x0 + n, *x1 = x0 + 2 * n, *s2 = x0 + 3 * n;
    const void* qkv = b.snap.qkv + (size_t)l * 3 * n * es;
    const void* attn = b.snap.attn + (size_t)l * n * es;
    const void* act = b.snap.act + (size_t)l * M * F * es;
    // LN2, linear2, ReLU, linear1
    VCAP_TRY(vcap_text_ln_bwd_dispatch(s2, b.g, pending, ly.ln2_g, d->ln_eps, M, E, b.ds, b.stats, y.ln2_g, y.ln2_b, s),
             "text_ln2_backward");
    if (int rc = dw_gemm(c, b.ds, E, act, 0, F, y.fc2_w, y.fc2_b, "text_linear2_weight_grad")) return rc;
    if (int rc = dx_gemm(c, b.ds, wt.fc2_t, b.wide, F, E, "text_linear2_backward")) return rc;
    VCAP_TRY(vcap_text_relu_bwd_dispatch(dt, act, (long)M * F, b.wide, s), "text_relu_backward");
    if (int rc = dw_gemm(c, b.wide, F, x1, 1, E, y.fc1_w, y.fc1_b, "text_linear1_weight_grad")) return rc;
    if (int rc = dx_gemm(c, b.wide, wt.fc1_t, b.d2, E, F, "text_linear1_backward")) return rc;
    // LN1, out_proj, attention, in_proj
    VCAP_TRY(vcap_text_ln_bwd_dispatch(s1, b.ds, b.d2, ly.ln1_g, d->ln_eps, M, E, b.g, b.stats, y.ln1_g, y.ln1_b, s),
             "text_ln1_backward");
    if (int rc = dw_gemm(c, b.g, E, attn, 0, E, y.out_w, y.out_b, "text_out_proj_weight_grad")) return rc;
    if (int rc = dx_gemm(c, b.g, wt.out_t, b.dO, E, E, "text_out_proj_backward")) return rc;
    VCAP_TRY(vcap_text_attn_bwd_dispatch(dt, qkv, b.dO, B, L, H, b.P, b.dS, b.wide, s), "text_attention_backward");
    if (int rc = dw_gemm(c, b.wide, 3 * E, x0, 1, E, y.in_w, y.in_b, "text_in_proj_weight_grad")) return rc;
    if (int rc = dx_gemm(c, b.wide, wt.in_t, b.d2, E, 3 * E, "text_in_proj_backward")) return rc;
    pending = b.d2;
  }
  VCAP_TRY(vcap_text_emb_grad_dispatch(ids, M, d->pad_id, d->vocab, b.g, pending, E, b.slot, grads->emb_ids,
                                       grads->emb_count, grads->emb_rows, s),
           "text_embedding_grad");
  return 0;
}

}  // extern "C"
