// The C ABI's (include/vcap.h) text-tower entry points: descriptor checks, workspace carving and the
// layer schedule in front of the kernels of text_encoder.hip and the rows GEMVs of decode.hip.  Every
// refusal returns before the first launch.
#include "runtime_common.h"

namespace {

struct TextBufs {
  float* x;    // [M, E] f32 residual stream
  void* xt;    // [M, E] T: the stream as the next GEMV's operand
  void* qkv;   // [M, 3E] T
  void* attn;  // [M, E] T
  void* act;   // [M, F] T
};

TextBufs carve_text(Carver& c, const vcap_text_desc* d, int B, int L) {
  const size_t M = (size_t)B * L, E = d->dim, es = esize(d->dtype);
  TextBufs b;
  b.x = (float*)c.take(M * E * 4);
  b.xt = c.take(M * E * es);
  b.qkv = c.take(M * 3 * E * es);
  b.attn = c.take(M * E * es);
  b.act = c.take(M * (size_t)d->ffn * es);
  return b;
}

}  // namespace

// descriptor and shape limits of vcap_text_encode (include/vcap.h); 0 when inside them
int vcap_text_limits(const vcap_text_desc* d, int B, int L, const char* who) {
  const std::string w = std::string(who) + ": ";
  if (!d) return fail(VCAP_E_ARG, w + "text desc is null");
  if (d->dtype != VCAP_DT_F32 && d->dtype != VCAP_DT_BF16)
    return fail(VCAP_E_ARG, w + "dtype must be VCAP_DT_F32 or VCAP_DT_BF16");
  if (d->dim <= 0 || d->n_head * 64 != d->dim) return fail(VCAP_E_UNSUPPORTED, w + "head_dim must be 64");
  if (d->dim % 128) return fail(VCAP_E_UNSUPPORTED, w + "dim must be a multiple of 128");
  if (d->dim > 1024) return fail(VCAP_E_UNSUPPORTED, w + "dim > 1024 (LayerNorm rows are held in registers)");
  if (d->ffn <= 0 || d->ffn % 128 || d->ffn > 4096)
    return fail(VCAP_E_UNSUPPORTED, w + "ffn must be a multiple of 128 in 128..4096");
  if (d->proj_dim % 64 || d->proj_dim < 64 || d->proj_dim > 1024)
    return fail(VCAP_E_UNSUPPORTED, w + "proj_dim must be a multiple of 64 in 64..1024");
  if (d->vocab <= 0 || d->pad_id < 0 || d->pad_id >= d->vocab)
    return fail(VCAP_E_ARG, w + "pad_id must be inside the vocabulary");
  if (d->n_layer < 0) return fail(VCAP_E_ARG, w + "n_layer < 0");
  if (B < 1) return fail(VCAP_E_ARG, w + "B must be at least 1");
  if (L < 1 || L > 64) return fail(VCAP_E_UNSUPPORTED, w + "L must be in 1..64");
  if ((long)B * L > vcap_gpt2_max_rows()) return fail(VCAP_E_UNSUPPORTED, w + "B*L exceeds vcap_gpt2_max_rows()");
  return 0;
}

// the pointer and alignment checks of a launch, after vcap_text_limits
int vcap_text_check_pointers(const vcap_text_desc* d, const void* workspace) {
  if (!d->emb || !d->proj_w || !d->proj_b || (d->n_layer > 0 && !d->layers))
    return fail(VCAP_E_ARG, "vcap_text_encode: emb / proj / layers pointer is null");
  for (int l = 0; l < d->n_layer; ++l) {
    const vcap_text_layer& ly = d->layers[l];
    if (!ly.in_w || !ly.in_b || !ly.out_w || !ly.out_b || !ly.ln1_g || !ly.ln1_b || !ly.fc1_w || !ly.fc1_b ||
        !ly.fc2_w || !ly.fc2_b || !ly.ln2_g || !ly.ln2_b)
      return fail(VCAP_E_ARG, "vcap_text_encode: layer " + std::to_string(l) + " has a null pointer");
  }
  if (((uintptr_t)d->emb & 15) || ((uintptr_t)d->proj_w & 15) || ((uintptr_t)workspace & 15))
    return fail(VCAP_E_UNSUPPORTED, "vcap_text_encode: emb, proj_w and the workspace must be 16-byte aligned");
  return 0;
}

// vcap_text_encode's launches.  With `snap` (the backward, runtime_text_grad.hip) layer l stores q | k | v, the
// attention output and the ReLU output in its own buffers instead of the shared ones, and the f32 stream
// is copied at the layer's input, after out_proj (the pre-LN1 sum), after LN1 and after linear2 (the
// pre-LN2 sum); the launches and their results are the same.  The final stream stays in the workspace's
// first M * E floats.
int vcap_text_forward(const vcap_text_desc* d, const int* ids, int B, int L, float* out, float* hidden_out,
                      void* workspace, const TextSnap* snap, hipStream_t s) {
  Carver cv(workspace);
  const TextBufs w = carve_text(cv, d, B, L);
  const int M = B * L, E = d->dim, F = d->ffn, dt = d->dtype;
  const size_t n = (size_t)M * E, es = esize(dt);
  auto keep = [&](int l, int which) -> hipError_t {   // copy of the f32 stream for the backward
    if (!snap) return hipSuccess;
    return hipMemcpyAsync(snap->x + ((size_t)l * 4 + which) * n, w.x, n * 4, hipMemcpyDeviceToDevice, s);
  };
  VCAP_TRY(vcap_text_gather_dispatch(dt, ids, M, d->emb, d->vocab, E, w.x, w.xt, s), "text_gather");
  for (int l = 0; l < d->n_layer; ++l) {
    const vcap_text_layer& ly = d->layers[l];
    void* qkv = snap ? (void*)(snap->qkv + (size_t)l * 3 * n * es) : w.qkv;
    void* attn = snap ? (void*)(snap->attn + (size_t)l * n * es) : w.attn;
    void* act = snap ? (void*)(snap->act + (size_t)l * M * F * es) : w.act;
    VCAP_TRY(keep(l, 0), "text snapshot");
    // 1) in_proj -> q | k | v rows.  No launch of the tower plans a K split (sk_part / sk_cnt stay null).
    RowsGemmArgs a{};
    a.M = M; a.x = w.xt; a.ldx = E; a.w = ly.in_w; a.bias = ly.in_b; a.N = 3 * E; a.K = E;
    a.out = qkv; a.ldo = 3 * E;
    VCAP_TRY(vcap_rows_gemm_dispatch(dt, PRO_DIRECT, EPI_STORE, a, nullptr, s), "text_in_proj");
    // 2) bidirectional attention, no mask
    VCAP_TRY(vcap_text_attention_dispatch(dt, qkv, attn, B, L, d->n_head, s), "text_attention");
    // 3) x += out_proj(attn); x = LN1(x)
    RowsGemmArgs b{};
    b.M = M; b.x = attn; b.ldx = E; b.w = ly.out_w; b.bias = ly.out_b; b.N = E; b.K = E;
    b.out = w.x; b.ldo = E;
    VCAP_TRY(vcap_rows_gemm_dispatch(dt, PRO_DIRECT, EPI_RESID, b, nullptr, s), "text_out_proj");
    VCAP_TRY(keep(l, 1), "text snapshot");
    VCAP_TRY(vcap_text_resid_ln_dispatch(dt, w.x, w.xt, ly.ln1_g, ly.ln1_b, M, E, d->ln_eps, s), "text_ln1");
    VCAP_TRY(keep(l, 2), "text snapshot");
    // 4) act = relu(linear1(x)); x += linear2(act); x = LN2(x)
    RowsGemmArgs c{};
    c.M = M; c.x = w.xt; c.ldx = E; c.w = ly.fc1_w; c.bias = ly.fc1_b; c.N = F; c.K = E;
    c.out = act; c.ldo = F;
    VCAP_TRY(vcap_rows_gemm_dispatch(dt, PRO_DIRECT, EPI_RELU, c, nullptr, s), "text_linear1");
    RowsGemmArgs e{};
    e.M = M; e.x = act; e.ldx = F; e.w = ly.fc2_w; e.bias = ly.fc2_b; e.N = E; e.K = F;
    e.out = w.x; e.ldo = E;
    VCAP_TRY(vcap_rows_gemm_dispatch(dt, PRO_DIRECT, EPI_RESID, e, nullptr, s), "text_linear2");
    VCAP_TRY(keep(l, 3), "text snapshot");
    VCAP_TRY(vcap_text_resid_ln_dispatch(dt, w.x, w.xt, ly.ln2_g, ly.ln2_b, M, E, d->ln_eps, s), "text_ln2");
  }
  if (hidden_out)
    VCAP_TRY(hipMemcpyAsync(hidden_out, w.x, (size_t)M * E * 4, hipMemcpyDeviceToDevice, s), "text hidden_out copy");
  VCAP_TRY(vcap_text_pool_dispatch(w.x, ids, d->pad_id, B, L, E, d->proj_w, d->proj_b, d->proj_dim, out, s),
           "text_pool");
  return 0;
}

extern "C" {

size_t vcap_text_workspace_bytes(const vcap_text_desc* d, int B, int L) {
  if (vcap_text_limits(d, B, L, "vcap_text_workspace_bytes")) return 0;
  return carved_bytes([&](Carver& c) { carve_text(c, d, B, L); });
}

int vcap_text_encode(const vcap_text_desc* d, const int* ids, int B, int L, float* out, float* hidden_out,
                     void* workspace, size_t ws_bytes, void* stream) {
  if (int rc = vcap_text_limits(d, B, L, "vcap_text_encode")) return rc;
  if (!ids || !out || !workspace) return fail(VCAP_E_ARG, "vcap_text_encode: null pointer");
  if (int rc = vcap_text_check_pointers(d, workspace)) return rc;
  if (ws_bytes < carved_bytes([&](Carver& c) { carve_text(c, d, B, L); }))
    return fail(VCAP_E_WORKSPACE, "vcap_text_encode: workspace too small (vcap_text_workspace_bytes)");
  return vcap_text_forward(d, ids, B, L, out, hidden_out, workspace, nullptr, (hipStream_t)stream);
}

}  // extern "C"
