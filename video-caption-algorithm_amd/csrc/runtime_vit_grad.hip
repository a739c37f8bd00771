// vcap_vit_encode_backward and vcap_vit_attention_backward (include/vcap.h): the gradient of a scalar of the
// encoder output with respect to encoder.proj, the final norm, every tensor of the last n_tail blocks and, with
// n_tail == depth, the patch embedding, the class token and the positional table.  The forward is
// vcap_vit_encode's schedule (runtime_vit.hip vcap_vit_forward) keeping, per unfrozen block, the f32 stream at
// the block input (x0) and after the attention residual (x1), q | k | v, the attention output and the GELU
// output; the backward walks the unfrozen blocks last to first and stops at the first one's input.
//
// Per pre-LN block, g = the gradient at the block output x2 = x1 + fc2(gelu(u)), u = fc1(LN2(x1)),
// x1 = x0 + proj(attn(qkv(LN1(x0)))):
//   xn2 = LN2(x1) and u = fc1(xn2) + b are recomputed (u in f32: the fc1 GEMM without its GELU epilogue)
//   dfc2:  db = colsum(g), dW = g^T . act, dact = g . W2;  du = dact gelu'(u)
//   dfc1:  db = colsum(du), dW = du^T . xn2, dxn2 = du . W1
//   g     += dLN2(x1) . dxn2          dgamma2, dbeta2            (g is now the gradient at x1)
//   dproj: db = colsum(g), dW = g^T . attn, dO = g . Wp;  dq | dk | dv = attention backward
//   dqkv:  db = colsum(dqkv), dW = dqkv^T . xn1 (xn1 = LN1(x0) recomputed), dxn1 = dqkv . Wqkv
//   g     += dLN1(x0) . dxn1          dgamma1, dbeta1            (g is now the gradient at x0)
// The last block ran its post-attention half on the B*T class-token rows only, so its fc2 / fc1 / LN2 / proj
// steps run on those rows in compact form; dO and g are then scattered to the CLS rows of zeroed full buffers.
// dx products: C = A . Wt^T on vcap_grad_gemm_kernel over the grad desc's transposed weights, one pass over K.
// dW products: vcap_vit_xty_kernel over 256-row slabs added in slab order.  Kernels, rounding points, orders
// and the exact-zero argument: vit_backward.hip.
#include <algorithm>

#include "runtime_common.h"

namespace {

constexpr int kDwSlabRows = 256;   // rows of M per slab of a weight gradient
constexpr long kMaxFrameHeads = 65535;   // (frame, head) pairs of one call: grid.y / grid.z of the attention backward
constexpr long kMaxRows = 1L << 22;       // B * T * tokens of one call: keeps every grid.y / grid.z (row tiles, slabs) in range

// the call's launch grids: (frame, head) pairs and rows
bool grids_ok(const vcap_vit_desc* d, int B, int T) {
  const long g = d->image / d->patch, BT = (long)B * T;
  return BT * d->heads <= kMaxFrameHeads && BT * (g * g + 1) <= kMaxRows;
}

int dw_slabs(long M) { return (int)((M + kDwSlabRows - 1) / kDwSlabRows); }

struct AttnBwdBufs {
  void* dO;    // [M][D] T: dO as an MFMA operand (bf16 only; f32 reads the caller's)
  void* P;     // [BT*H][ldp][ldp] T
  void* dS;
  void* dST;
};

AttnBwdBufs carve_attn_bwd(Carver& c, int dt, int BT, int N, int H) {
  const size_t ldp = vcap_vit_attn_bwd_ldp(N), mat = (size_t)BT * H * ldp * ldp * esize(dt);
  AttnBwdBufs b;
  b.dO = c.take(dt == VCAP_DT_BF16 ? (size_t)BT * N * H * 64 * 2 : 0);
  b.P = c.take(mat);
  b.dS = c.take(mat);
  b.dST = c.take(mat);
  return b;
}

int attn_bwd(int dt, const void* qkv, const float* dO, float* dqkv, int BT, int N, int H, const AttnBwdBufs& b,
             hipStream_t s) {
  const void* o = dO;
  if (dt == VCAP_DT_BF16) {
    VCAP_TRY(vcap_grad_to_bf16_dispatch(dO, (long)BT * N * H * 64, b.dO, s), "vit_attention_backward");
    o = b.dO;
  }
  VCAP_TRY(vcap_vit_attn_bwd_dispatch(dt, qkv, o, BT, N, H, b.P, b.dS, b.dST, dqkv, s), "vit_attention_backward");
  return 0;
}

struct VitGradBufs {
  void* fwd;        // vcap_vit_encode's workspace
  VitSnap snap;
  float* xc;        // [BT][D] the final stream's CLS rows, compact
  float* xnc;       // [BT][D] their final norm
  float* pooled;    // [B][D]
  float* gc;        // [BT][D] the gradient at the CLS rows (final norm, the last block's compact half)
  float* dc;        // [BT][D] a compact dx product
  float* g;         // [M][D] the residual gradient
  float* dx;        // [M][D] a dx product: dxn2, dO, dxn1
  float* u;         // [M][mlp] f32 pre-activation
  float* wa;        // [M][max(mlp, 3D)] dact, dq | dk | dv, the patch rows of g
  float* wb;        // [M][mlp] du
  void* opr;        // [M][max(mlp, 3D)] T: a row gradient as a bf16 operand
  float* stats;     // [M][2]
  float* slabs;     // the running weight gradient's slabs
  AttnBwdBufs at;
};

VitGradBufs carve_vit_grad(Carver& c, const vcap_vit_desc* d, int B, int T, int n_tail) {
  const int g = d->image / d->patch, N = g * g + 1;
  const size_t BT = (size_t)B * T, M = BT * N, D = d->dim, F = d->mlp, es = esize(d->dtype), nt = n_tail;
  const size_t W = std::max(F, 3 * D);
  VitGradBufs b;
  b.fwd = c.take(vcap_vit_workspace_bytes(d, B, T));
  b.snap.n_tail = n_tail;
  b.snap.x0 = (float*)c.take(nt * M * D * 4);
  b.snap.x1 = (float*)c.take(nt * M * D * 4);
  b.snap.qkv = (char*)c.take(nt * M * 3 * D * es);
  b.snap.attn = (char*)c.take(nt * M * D * es);
  b.snap.act = (char*)c.take(nt * M * F * es);
  b.snap.x = nullptr;
  b.snap.xn = b.snap.patches = nullptr;
  b.xc = (float*)c.take(BT * D * 4);
  b.xnc = (float*)c.take(BT * D * 4);
  b.pooled = (float*)c.take((size_t)B * D * 4);
  b.gc = (float*)c.take(BT * D * 4);
  b.dc = (float*)c.take(BT * D * 4);
  b.g = (float*)c.take(M * D * 4);
  b.dx = (float*)c.take(M * D * 4);
  b.u = (float*)c.take(M * F * 4);
  b.wa = (float*)c.take(M * W * 4);
  b.wb = (float*)c.take(M * F * 4);
  b.opr = c.take(M * W * es);
  b.stats = (float*)c.take(M * 2 * 4);
  const size_t biggest = std::max({3 * D * D, D * F, D * (size_t)d->kpad});
  b.slabs = (float*)c.take(biggest * dw_slabs((long)M) * 4);
  b.at = carve_attn_bwd(c, d->dtype, (int)BT, N, d->heads);
  return b;
}

// what the backward serves beyond the forward's limits; the workspace query returns 0 outside them
int check_vit_grad(const vcap_vit_desc* d, const vcap_vit_grad_desc* g, int B, int T, int n_tail, const char* who) {
  if (int rc = vcap_vit_check(d)) return rc;
  if (d->dtype != VCAP_DT_F32 && d->dtype != VCAP_DT_BF16)
    return fail(VCAP_E_UNSUPPORTED, std::string(who) + ": operand dtype must be VCAP_DT_F32 or VCAP_DT_BF16");
  if (d->dim % 128 || d->mlp % 128)
    return fail(VCAP_E_UNSUPPORTED, std::string(who) + ": dim and mlp must be multiples of 128");
  if (!g) return fail(VCAP_E_ARG, std::string(who) + ": grad desc is null");
  if (g->dtype != d->dtype || g->dim != d->dim || g->mlp != d->mlp || g->depth != d->depth)
    return fail(VCAP_E_ARG, std::string(who) + ": grad desc dtype / dim / mlp / depth differ from the vit desc's");
  if (B <= 0 || T <= 0) return fail(VCAP_E_ARG, std::string(who) + ": B and T must be positive");
  if (n_tail < 1 || n_tail > d->depth) return fail(VCAP_E_ARG, std::string(who) + ": n_tail outside 1 .. depth");
  if (!grids_ok(d, B, T))
    return fail(VCAP_E_UNSUPPORTED, std::string(who) + ": B * T * heads > 65535 or B * T * tokens > 2^22 (send the clips in chunks)");
  return 0;
}

struct Ctx {
  int dt;
  const VitGradBufs* b;
  hipStream_t s;
};

// the row gradient A [rows, K] f32 as an MFMA operand: itself (f32) or its bf16 copy in opr
int operand(const Ctx& c, const float* A, long n, const void** out, const char* where) {
  *out = A;
  if (c.dt == VCAP_DT_BF16) {
    VCAP_TRY(vcap_grad_to_bf16_dispatch(A, n, c.b->opr, c.s), where);
    *out = c.b->opr;
  }
  return 0;
}

// C [rows, N] f32 = A [rows, K] . Wt [N, K]^T
int dx_gemm(const Ctx& c, const void* A, const void* Wt, float* C, int rows, int N, int K, const char* where) {
  VCAP_TRY(vcap_grad_gemm_dispatch(c.dt, A, K, Wt, K, C, N, rows, N, K, 0, c.s), where);
  return 0;
}

// dW [R, N] f32 = dY^T . X over `rows` rows; dY [rows, R] and X [rows, ldx >= N] in the operand dtype
int dw_gemm(const Ctx& c, const void* dY, int R, const void* X, long ldx, int N, int rows, float* dW, const char* where) {
  const int ns = dw_slabs(rows);
  XtyArgs a{};
  a.X = dY;
  a.ldx = R;
  a.Kmem = R;
  a.Y = X;
  a.ldy = ldx;
  a.N = N;
  a.C = ns > 1 ? c.b->slabs : dW;
  a.ldc = N;
  a.K = R;
  a.rows_total = rows;
  a.slab_rows = kDwSlabRows;
  a.slab_step = kDwSlabRows;
  a.Z2 = 1;
  a.xs1 = (long)kDwSlabRows * R;
  a.ys1 = (long)kDwSlabRows * ldx;
  a.cs1 = (long)R * N;
  VCAP_TRY(vcap_vit_xty_dispatch(c.dt, a, ns, c.s), where);
  if (ns > 1) VCAP_TRY(vcap_grad_slab_sum_dispatch(c.b->slabs, (long)R * N, ns, nullptr, N, 0, dW, c.s), where);
  return 0;
}

}  // namespace

extern "C" {

size_t vcap_vit_attention_backward_workspace_bytes(int dtype, int frames, int tokens, int heads) {
  if ((dtype != VCAP_DT_F32 && dtype != VCAP_DT_BF16) || frames <= 0 || tokens < 1 || tokens > 288 || heads <= 0 ||
      (long)frames * heads > kMaxFrameHeads)
    return 0;
  return carved_bytes([&](Carver& c) { carve_attn_bwd(c, dtype, frames, tokens, heads); });
}

int vcap_vit_attention_backward(int dtype, const void* qkv, const float* dout, float* dqkv, int frames, int tokens,
                                int heads, void* workspace, void* stream) {
  if (!qkv || !dout || !dqkv || !workspace || frames <= 0 || tokens <= 0 || heads <= 0)
    return fail(VCAP_E_ARG, "vcap_vit_attention_backward: bad arguments");
  if (dtype != VCAP_DT_F32 && dtype != VCAP_DT_BF16)
    return fail(VCAP_E_UNSUPPORTED, "vcap_vit_attention_backward: dtype must be VCAP_DT_F32 or VCAP_DT_BF16");
  if (tokens > 288) return fail(VCAP_E_UNSUPPORTED, "vcap_vit_attention_backward: tokens > 288");
  if ((long)frames * heads > kMaxFrameHeads)
    return fail(VCAP_E_UNSUPPORTED, "vcap_vit_attention_backward: frames * heads > 65535");
  if (((uintptr_t)qkv & 15) || ((uintptr_t)dout & 15) || ((uintptr_t)dqkv & 15) || ((uintptr_t)workspace & 255))
    return fail(VCAP_E_UNSUPPORTED, "vcap_vit_attention_backward: pointers must be 16-byte aligned (workspace: 256)");
  Carver c(workspace);
  const AttnBwdBufs b = carve_attn_bwd(c, dtype, frames, tokens, heads);
  return attn_bwd(dtype, qkv, dout, dqkv, frames, tokens, heads, b, (hipStream_t)stream);
}

size_t vcap_vit_backward_workspace_bytes(const vcap_vit_desc* d, int B, int T, int n_tail) {
  if (!d || vcap_vit_check(d) || (d->dtype != VCAP_DT_F32 && d->dtype != VCAP_DT_BF16) || d->dim % 128 ||
      d->mlp % 128 || B <= 0 || T <= 0 || n_tail < 1 || n_tail > d->depth || !grids_ok(d, B, T))
    return 0;
  return carved_bytes([&](Carver& c) { carve_vit_grad(c, d, B, T, n_tail); });
}

int vcap_vit_encode_backward(const vcap_vit_desc* d, const vcap_vit_grad_desc* gd, const float* frames, int B, int T,
                             int n_tail, const float* grad_out, float* enc_out, const vcap_vit_param_grads* grads,
                             void* workspace, size_t ws_bytes, void* stream) {
  const char* who = "vcap_vit_encode_backward";
  if (int rc = check_vit_grad(d, gd, B, T, n_tail, who)) return rc;
  if (!frames || !grad_out || !enc_out || !grads || !workspace || !gd->layers || !grads->layers)
    return fail(VCAP_E_ARG, "vcap_vit_encode_backward: null pointer");
  if (!grads->proj_w || !grads->proj_b || !grads->norm_g || !grads->norm_b)
    return fail(VCAP_E_ARG, "vcap_vit_encode_backward: a head gradient pointer is null");
  const bool full = n_tail == d->depth;
  if (full && (!grads->patch_w || !grads->patch_b || !grads->cls || !grads->pos))
    return fail(VCAP_E_ARG, "vcap_vit_encode_backward: n_tail == depth needs the patch_w / patch_b / cls / pos gradients");
  if (full && ((uintptr_t)grads->patch_w & 15))
    return fail(VCAP_E_UNSUPPORTED, "vcap_vit_encode_backward: weight gradients must be 16-byte aligned");
  const int first = d->depth - n_tail;
  for (int j = 0; j < n_tail; ++j) {
    const vcap_vit_grad_layer& w = gd->layers[first + j];
    const vcap_vit_param_grads_layer& y = grads->layers[j];
    if (!w.qkv_t || !w.proj_t || !w.fc1_t || !w.fc2_t)
      return fail(VCAP_E_ARG, "vcap_vit_encode_backward: grad desc block " + std::to_string(first + j) + " has a null pointer");
    if (!y.ln1_g || !y.ln1_b || !y.qkv_w || !y.qkv_b || !y.proj_w || !y.proj_b || !y.ln2_g || !y.ln2_b || !y.fc1_w ||
        !y.fc1_b || !y.fc2_w || !y.fc2_b)
      return fail(VCAP_E_ARG, "vcap_vit_encode_backward: a gradient pointer of block " + std::to_string(first + j) + " is null");
    if (((uintptr_t)w.qkv_t & 15) || ((uintptr_t)w.proj_t & 15) || ((uintptr_t)w.fc1_t & 15) || ((uintptr_t)w.fc2_t & 15) ||
        ((uintptr_t)y.qkv_w & 15) || ((uintptr_t)y.proj_w & 15) || ((uintptr_t)y.fc1_w & 15) || ((uintptr_t)y.fc2_w & 15))
      return fail(VCAP_E_UNSUPPORTED, "vcap_vit_encode_backward: weight copies and weight gradients must be 16-byte aligned");
  }
  if ((uintptr_t)workspace & 255) return fail(VCAP_E_UNSUPPORTED, "vcap_vit_encode_backward: workspace must be 256-byte aligned");
  if (ws_bytes < vcap_vit_backward_workspace_bytes(d, B, T, n_tail))
    return fail(VCAP_E_WORKSPACE, "vcap_vit_encode_backward: workspace too small (vcap_vit_backward_workspace_bytes)");

  hipStream_t s = (hipStream_t)stream;
  Carver cv(workspace);
  VitGradBufs b = carve_vit_grad(cv, d, B, T, n_tail);
  const int dt = d->dtype, D = d->dim, F = d->mlp, H = d->heads, gr = d->image / d->patch, P = gr * gr, N = P + 1;
  const int BT = B * T, M = BT * N, VD = d->video_dim;
  const size_t es = esize(dt);
  const Ctx c{dt, &b, s};

  if (int rc = vcap_vit_forward(d, nullptr, frames, B, T, enc_out, nullptr, b.fwd, &b.snap, s)) return rc;
  void* xn = b.snap.xn;   // [M][D] T: the forward's LayerNorm output buffer, free now

  // head: encoder.proj, the temporal mean, the final norm on the CLS rows
  VCAP_TRY(vcap_vit_rows_copy_dispatch(b.snap.x, (long)N * D, b.xc, D, BT, D, s), "vit_head_backward");
  VCAP_TRY(vcap_layernorm_dispatch(VCAP_DT_F32, b.xc, D, b.xnc, D, d->norm_g, d->norm_b, BT, D, d->ln_eps, s),
           "vit_head_backward");
  VCAP_TRY(vcap_vit_head_bwd_dispatch(b.xnc, B, T, D, grad_out, d->proj_w, VD, b.pooled, b.dc, grads->proj_w,
                                      grads->proj_b, s),
           "vit_head_backward");
  VCAP_TRY(vcap_text_ln_bwd_dispatch(b.xc, b.dc, nullptr, d->norm_g, d->ln_eps, BT, D, b.gc, b.stats, grads->norm_g,
                                     grads->norm_b, s),
           "vit_norm_backward");

  for (int l = d->depth - 1; l >= first; --l) {
    const int j = l - first;
    const bool last = l == d->depth - 1;
    const int Mt = last ? BT : M;
    const vcap_vit_layer& ly = d->layers[l];
    const vcap_vit_grad_layer& wt = gd->layers[l];
    const vcap_vit_param_grads_layer& y = grads->layers[j];
    const float* x0 = b.snap.x0 + (size_t)j * M * D;
    const float* x1 = b.snap.x1 + (size_t)j * M * D;
    const void* qkv = b.snap.qkv + (size_t)j * M * 3 * D * es;
    const void* attn = b.snap.attn + (size_t)j * M * D * es;
    const void* act = b.snap.act + (size_t)j * M * F * es;
    float* g = last ? b.gc : b.g;       // the gradient at the block output, on the rows its MLP half ran on
    float* dxr = last ? b.dc : b.dx;
    const void* a = nullptr;
    // the MLP half: recompute xn2 and the f32 pre-activation, then fc2, GELU, fc1, LN2
    VCAP_TRY(vcap_layernorm_dispatch(dt, x1, D, xn, D, ly.ln2_g, ly.ln2_b, Mt, D, d->ln_eps, s), "vit_norm2_recompute");
    GemmEpi eu{};
    eu.bias = ly.fc1_b;
    VCAP_TRY(vcap_gemm_dispatch(dt, VCAP_DT_F32, xn, D, ly.fc1_w, D, b.u, F, Mt, F, D, eu, s), "vit_fc1_recompute");
    VCAP_TRY(vcap_text_colsum_dispatch(g, Mt, D, y.fc2_b, s), "vit_fc2_bias_grad");
    if (int rc = operand(c, g, (long)Mt * D, &a, "vit_fc2_backward")) return rc;
    if (int rc = dw_gemm(c, a, D, act, F, F, Mt, y.fc2_w, "vit_fc2_weight_grad")) return rc;
    if (int rc = dx_gemm(c, a, wt.fc2_t, b.wa, Mt, F, D, "vit_fc2_backward")) return rc;
    VCAP_TRY(vcap_gelu_backward_dispatch(VCAP_DT_F32, b.u, b.wa, (long)Mt * F, b.wb, s), "vit_gelu_backward");
    VCAP_TRY(vcap_text_colsum_dispatch(b.wb, Mt, F, y.fc1_b, s), "vit_fc1_bias_grad");
    if (int rc = operand(c, b.wb, (long)Mt * F, &a, "vit_fc1_backward")) return rc;
    if (int rc = dw_gemm(c, a, F, xn, D, D, Mt, y.fc1_w, "vit_fc1_weight_grad")) return rc;
    if (int rc = dx_gemm(c, a, wt.fc1_t, dxr, Mt, D, F, "vit_fc1_backward")) return rc;
    VCAP_TRY(vcap_ln_backward_stats_dispatch(x1, dxr, ly.ln2_g, d->ln_eps, Mt, D, g, b.stats, s), "vit_norm2_backward");
    VCAP_TRY(vcap_ln_colsum_dispatch(dxr, x1, b.stats, Mt, D, y.ln2_g, y.ln2_b, s), "vit_norm2_backward");
    // the attention half: proj, attention, qkv, LN1
    VCAP_TRY(vcap_text_colsum_dispatch(g, Mt, D, y.proj_b, s), "vit_proj_bias_grad");
    if (int rc = operand(c, g, (long)Mt * D, &a, "vit_proj_backward")) return rc;
    if (int rc = dw_gemm(c, a, D, attn, D, D, Mt, y.proj_w, "vit_proj_weight_grad")) return rc;
    if (int rc = dx_gemm(c, a, wt.proj_t, dxr, Mt, D, D, "vit_proj_backward")) return rc;
    if (last) {   // back to all M rows: zero everywhere but the class-token rows
      VCAP_TRY(hipMemsetAsync(b.dx, 0, (size_t)M * D * 4, s), "vit_cls_scatter");
      VCAP_TRY(hipMemsetAsync(b.g, 0, (size_t)M * D * 4, s), "vit_cls_scatter");
      VCAP_TRY(vcap_vit_rows_copy_dispatch(b.dc, D, b.dx, (long)N * D, BT, D, s), "vit_cls_scatter");
      VCAP_TRY(vcap_vit_rows_copy_dispatch(b.gc, D, b.g, (long)N * D, BT, D, s), "vit_cls_scatter");
    }
    if (int rc = attn_bwd(dt, qkv, b.dx, b.wa, BT, N, H, b.at, s)) return rc;
    VCAP_TRY(vcap_layernorm_dispatch(dt, x0, D, xn, D, ly.ln1_g, ly.ln1_b, M, D, d->ln_eps, s), "vit_norm1_recompute");
    VCAP_TRY(vcap_text_colsum_dispatch(b.wa, M, 3 * D, y.qkv_b, s), "vit_qkv_bias_grad");
    if (int rc = operand(c, b.wa, (long)M * 3 * D, &a, "vit_qkv_backward")) return rc;
    if (int rc = dw_gemm(c, a, 3 * D, xn, D, D, M, y.qkv_w, "vit_qkv_weight_grad")) return rc;
    if (int rc = dx_gemm(c, a, wt.qkv_t, b.dx, M, D, 3 * D, "vit_qkv_backward")) return rc;
    VCAP_TRY(vcap_ln_backward_stats_dispatch(x0, b.dx, ly.ln1_g, d->ln_eps, M, D, b.g, b.stats, s), "vit_norm1_backward");
    VCAP_TRY(vcap_ln_colsum_dispatch(b.dx, x0, b.stats, M, D, y.ln1_g, y.ln1_b, s), "vit_norm1_backward");
  }
  if (full) {   // b.g is the gradient at the embedding output x[bt][0] = cls + pos[0], x[bt][1 + p] = patch + pos
    VCAP_TRY(vcap_vit_pos_grad_dispatch(b.g, BT, N, D, grads->pos, grads->cls, s), "vit_pos_grad");
    VCAP_TRY(vcap_vit_rows_copy_dispatch(b.g + D, (long)N * D, b.wa, (long)P * D, BT, (long)P * D, s), "vit_patch_grad");
    VCAP_TRY(vcap_text_colsum_dispatch(b.wa, BT * P, D, grads->patch_b, s), "vit_patch_bias_grad");
    const void* a = nullptr;
    if (int rc = operand(c, b.wa, (long)BT * P * D, &a, "vit_patch_grad")) return rc;
    if (int rc = dw_gemm(c, a, D, b.snap.patches, d->kpad, d->kpad, BT * P, grads->patch_w, "vit_patch_weight_grad"))
      return rc;
  }
  return 0;
}

}  // extern "C"
