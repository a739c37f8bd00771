// The ViT side of the C ABI (include/vcap.h): descriptor checks, workspace carving, the encoder's
// forward schedule (the reference drives it from Python, timm forward_features; here one ABI call issues
// the whole encode) and the single-operator entry points the tests and tools call.
#include "runtime_common.h"

namespace {

struct VitBufs {
  float* x;
  void* xn;
  void* qkv;
  void* attn;
  void* act;
  uint8_t* xn_s;   // MXFP8 scales of xn / act
  uint8_t* act_s;
  float* splitk;   // split-K partial slabs of the CLS-tail attn-proj / fc2 (deterministic reduce)
  size_t splitk_bytes;
};

// operand dtype of patch-embed / qkv output / attention / attn-proj: bf16 in the MXFP8 mode
int vit_adt(int dt) { return dt == VCAP_DT_MXFP8 ? VCAP_DT_BF16 : dt; }

VitBufs carve_vit(Carver& c, const vcap_vit_desc* d, int B, int T) {
  const int tokens = (d->image / d->patch) * (d->image / d->patch) + 1;
  const size_t M = (size_t)B * T * tokens;
  const size_t es = esize(d->dtype), ea = esize(vit_adt(d->dtype));
  const size_t npatch = (size_t)B * T * (tokens - 1);
  VitBufs v;
  // MXFP8 mode: any GEMM of a layer may stay bf16 (its weight scales NULL), so the LayerNorm and
  // fc1 outputs are sized for bf16 elements
  const size_t en = es > ea ? es : ea;
  v.x = (float*)c.take(M * d->dim * 4);
  v.xn = c.take(M * d->dim * en);
  v.qkv = c.take(M * 3 * d->dim * ea);
  v.attn = c.take(M * d->dim * ea);
  size_t act = M * d->mlp * en;
  const size_t patches = npatch * d->kpad * ea;
  v.act = c.take(act > patches ? act : patches);
  v.xn_s = v.act_s = nullptr;
  v.splitk_bytes = (size_t)16 * B * T * d->dim * 4;   // <= 16 splits of the [B*T, dim] CLS rows
  v.splitk = (float*)c.take(v.splitk_bytes);
  if (d->dtype == VCAP_DT_MXFP8) {
    v.xn_s = (uint8_t*)c.take(mx_scale_bytes((int)M, d->dim));
    v.act_s = (uint8_t*)c.take(mx_scale_bytes((int)M, d->mlp));
  }
  return v;
}

int check_vit(const vcap_vit_desc* d) {
  if (!d || !d->layers) return fail(VCAP_E_ARG, "vit desc is null");
  if (d->dtype != VCAP_DT_F32 && d->dtype != VCAP_DT_BF16 && d->dtype != VCAP_DT_MXFP8 && d->dtype != VCAP_DT_F16)
    return fail(VCAP_E_ARG, "vit dtype");
  if (d->heads * 64 != d->dim) return fail(VCAP_E_UNSUPPORTED, "vit head_dim must be 64");
  const int ka = vcap_gemm_k_align(d->dtype);
  if (d->dim % ka || d->mlp % ka || d->kpad % vcap_gemm_k_align(vit_adt(d->dtype)) || d->kpad < 3 * d->patch * d->patch)
    return fail(VCAP_E_UNSUPPORTED, "vit dims must be multiples of the GEMM K step");
  if (d->dtype == VCAP_DT_MXFP8) {
    // per GEMM: weight scales present = MXFP8 block GEMM, NULL = that GEMM's weights are bf16
    if (d->dim > 1024) return fail(VCAP_E_UNSUPPORTED, "MXFP8 LayerNorm holds rows of <= 1024 in registers");
    if (d->dim % 256 || d->mlp % 256) return fail(VCAP_E_UNSUPPORTED, "MXFP8 dims must be multiples of 256");
  }
  if (d->image % d->patch) return fail(VCAP_E_ARG, "image not divisible by patch");
  const int tokens = (d->image / d->patch) * (d->image / d->patch) + 1;
  if (tokens > 288) return fail(VCAP_E_UNSUPPORTED, "more than 288 tokens");
  // what the encode would otherwise meet after its first launches: a token count the attention dispatcher
  // has no kernel for in this dtype, and rows the head / prefix kernels cannot hold
  if (!vcap_vit_attention_supported(vit_adt(d->dtype), tokens))
    return fail(VCAP_E_UNSUPPORTED, "vit attention serves 33..192 and 225..256 tokens in fp16 only");
  if (!vcap_vit_head_prefix_supported(d->dim, 1)) return fail(VCAP_E_UNSUPPORTED, "vit dim > 1024 (the head holds a row in LDS)");
  if (!vcap_vit_head_prefix_supported(1, d->video_dim)) return fail(VCAP_E_UNSUPPORTED, "video_dim > 1024");
  return 0;
}

// block `ly` runs QKV + attention as one kernel: bf16 operands (neither QKV nor attn-proj in MXFP8) at a
// token count the fused kernel takes
bool vit_layer_fused(const vcap_vit_desc* d, const vcap_vit_layer& ly) {
  const bool mx = d->dtype == VCAP_DT_MXFP8;
  const int g = d->image / d->patch;
  return !(mx && ly.qkv_ws) && !(mx && ly.proj_ws) && vcap_vit_qkv_attention_supported(vit_adt(d->dtype), g * g + 1, d->heads);
}

// probe site of a block's launch: the last block's CLS-row launches are priced apart ("vit.fc1.cls")
std::string vit_site(const char* name, bool last) { return std::string("vit.") + name + (last ? ".cls" : ""); }

}  // namespace

extern "C" {

int vcap_vit_attention(int dtype, const void* qkv, void* out, int frames, int tokens, int heads, void* stream) {
  if (!qkv || !out || frames <= 0 || tokens <= 0 || heads <= 0) return fail(VCAP_E_ARG, "vcap_vit_attention: bad arguments");
  if (tokens > 288) return fail(VCAP_E_UNSUPPORTED, "vcap_vit_attention: tokens > 288");
  VCAP_TRY(vcap_vit_attention_dispatch(dtype, qkv, out, frames, tokens, heads, (hipStream_t)stream),
           "vcap_vit_attention");
  return 0;
}

int vcap_vit_qkv_attention_dt(int dtype, const void* xn, const void* wqkv, const float* bqkv, void* out, int frames,
                              int tokens, int heads, int cls_only, void* stream) {
  if (!xn || !wqkv || !bqkv || !out || frames <= 0 || tokens <= 0 || heads <= 0)
    return fail(VCAP_E_ARG, "vcap_vit_qkv_attention: bad arguments");
  if (dtype != VCAP_DT_BF16 && dtype != VCAP_DT_F16)
    return fail(VCAP_E_ARG, "vcap_vit_qkv_attention: dtype must be VCAP_DT_BF16 or VCAP_DT_F16");
  if (!vcap_vit_qkv_attention_supported(dtype, tokens, heads))
    return fail(VCAP_E_UNSUPPORTED, "vcap_vit_qkv_attention: needs 192 < tokens <= 208 (ViT-B/16) or 256 < tokens <= 272 (ViT-L/14) "
                "and heads*64 <= 4096");
  VCAP_TRY(vcap_vit_qkv_attention_dispatch(dtype, xn, wqkv, bqkv, out, frames, tokens, heads, cls_only ? 1 : 0,
                                           (hipStream_t)stream),
           "vcap_vit_qkv_attention");
  return 0;
}

int vcap_vit_qkv_attention(const void* xn, const void* wqkv, const float* bqkv, void* out, int frames, int tokens,
                           int heads, int cls_only, void* stream) {
  return vcap_vit_qkv_attention_dt(VCAP_DT_BF16, xn, wqkv, bqkv, out, frames, tokens, heads, cls_only, stream);
}

int vcap_vit_attention_mx(const void* qkv, void* out, uint8_t* out_scales, int frames, int tokens, int heads,
                          void* stream) {
  if (!qkv || !out || !out_scales || frames <= 0 || tokens <= 0 || heads <= 0)
    return fail(VCAP_E_ARG, "vcap_vit_attention_mx: bad arguments");
  if (tokens > 288) return fail(VCAP_E_UNSUPPORTED, "vcap_vit_attention_mx: tokens > 288");
  if ((heads * 64) % 256) return fail(VCAP_E_UNSUPPORTED, "vcap_vit_attention_mx: heads*64 must be a multiple of 256");
  if (!vcap_vit_attention_supported(VCAP_DT_BF16, tokens))
    return fail(VCAP_E_UNSUPPORTED, "vcap_vit_attention_mx: serves 1..32, 193..224 and 257..288 tokens");
  VCAP_TRY(vcap_vit_attention_mx_dispatch(qkv, out, out_scales, frames, tokens, heads, (hipStream_t)stream),
           "vcap_vit_attention_mx");
  return 0;
}

int vcap_vit_pool_temporal(int dtype, const void* feat, void* out, int bsz, int timesteps, int tokens, int channels,
                           int pool_gap, void* stream) {
  if (!feat || !out || bsz <= 0 || timesteps <= 0 || tokens <= 0 || channels <= 0)
    return fail(VCAP_E_ARG, "vcap_vit_pool_temporal: bad arguments");
  if (pool_gap && tokens <= 1) return fail(VCAP_E_ARG, "vcap_vit_pool_temporal: gap needs tokens > 1");
  VCAP_TRY(vcap_vit_pool_dispatch(dtype, feat, out, bsz, timesteps, tokens, channels, pool_gap, (hipStream_t)stream),
           "vcap_vit_pool_temporal");
  return 0;
}

int vcap_prefix_project(const float* emb, int B, int video_dim, const vcap_prefix_desc* pd, float* prefix_out,
                        void* stream) {
  if (!emb || !pd || !prefix_out || !pd->mapper_w || B <= 0) return fail(VCAP_E_ARG, "vcap_prefix_project: bad arguments");
  if (!vcap_vit_head_prefix_supported(1, video_dim)) return fail(VCAP_E_UNSUPPORTED, "video_dim > 1024");
  VCAP_TRY(vcap_vit_head_prefix_dispatch(nullptr, B, 1, 1, 1, nullptr, nullptr, 0.f, nullptr, nullptr, video_dim,
                                         pd->ln_scale, pd->in_weight, pd->mapper_w, pd->mapper_b,
                                         pd->prefix_len * pd->n_embd, nullptr, prefix_out, emb, nullptr,
                                         (hipStream_t)stream),
           "vcap_prefix_project");
  return 0;
}

size_t vcap_vit_workspace_bytes(const vcap_vit_desc* d, int B, int T) {
  return check_vit(d) ? 0 : carved_bytes([&](Carver& c) { carve_vit(c, d, B, T); });
}

int vcap_vit_layer_fuses_qkv_attention(const vcap_vit_desc* d, int layer) {
  if (int rc = check_vit(d)) return rc;
  if (layer < 0 || layer >= d->depth) return fail(VCAP_E_ARG, "vcap_vit_layer_fuses_qkv_attention: layer out of range");
  return vit_layer_fused(d, d->layers[layer]) ? 1 : 0;
}

int vcap_vit_encode(const vcap_vit_desc* d, const vcap_prefix_desc* pd, const float* frames, int B, int T,
                    float* enc_out, float* prefix_out, void* workspace, size_t ws_bytes, void* stream) {
  if (int rc = check_vit(d)) return rc;
  if (!frames || !enc_out || B <= 0 || T <= 0) return fail(VCAP_E_ARG, "vcap_vit_encode: bad arguments");
  if (prefix_out && (!pd || !pd->mapper_w)) return fail(VCAP_E_ARG, "vcap_vit_encode: prefix desc missing");
  if (ws_bytes < vcap_vit_workspace_bytes(d, B, T)) return fail(VCAP_E_WORKSPACE, "vcap_vit_encode: workspace too small");
  return vcap_vit_forward(d, pd, frames, B, T, enc_out, prefix_out, workspace, nullptr, (hipStream_t)stream);
}

}  // extern "C"

int vcap_vit_check(const vcap_vit_desc* d) { return check_vit(d); }

// vcap_vit_encode's schedule (arguments checked by the caller).  With `snap` (vcap_vit_encode_backward) the last
// snap->n_tail blocks keep what their backward reads: the f32 stream at the block input and after the attention
// residual is copied out, q | k | v, the attention output and the GELU output land in buffers of their own, and
// the QKV projection + attention run as the GEMM + attention pair (the fused kernel's bits,
// tests/test_gpu_qkv_attention.py) so that q | k | v reach HBM.  The blocks below run exactly as without it.
int vcap_vit_forward(const vcap_vit_desc* d, const vcap_prefix_desc* pd, const float* frames, int B, int T,
                     float* enc_out, float* prefix_out, void* workspace, VitSnap* snap, hipStream_t s) {
  Carver c(workspace);
  VitBufs w = carve_vit(c, d, B, T);
  const int dt = d->dtype, D = d->dim, g = d->image / d->patch, P = g * g, N = P + 1, BT = B * T;
  const int adt = vit_adt(dt);
  const bool mx = dt == VCAP_DT_MXFP8;
  const int M = BT * N;
  // LayerNorm of `rows` rows of x (ldx apart) into xn: MXFP8 with its scales when the GEMM it feeds is
  // MXFP8 (mxq), else the operand dtype
  auto norm = [&](bool mxq, long ldx, const float* gamma, const float* beta, int rows, const char* where) -> int {
    if (mxq)
      VCAP_TRY(vcap_layernorm_mx_dispatch(w.x, ldx, (uint8_t*)w.xn, w.xn_s, rows, gamma, beta, rows, D, d->ln_eps, s),
               where);
    else
      VCAP_TRY(vcap_layernorm_dispatch(adt, w.x, ldx, w.xn, D, gamma, beta, rows, D, d->ln_eps, s), where);
    return 0;
  };
  // patch embedding: im2col + GEMM whose epilogue adds bias + pos[1+p] and scatters row bt*N+1+p
  void* const patches = w.act;
  VCAP_TRY(vcap_patchify_dispatch(adt, frames, patches, w.x, d->cls, d->pos, BT, d->image, d->patch, d->kpad, N, D, s),
           "patchify");
  GemmEpi pe{d->patch_b, d->pos, D, 0, 2, P, N, 1, 1};
  VCAP_TRY(vcap_gemm_dispatch(adt, VCAP_DT_F32, patches, d->kpad, d->patch_w, d->kpad, w.x, D, BT * P, D, d->kpad, pe, s),
           "patch_gemm");
  for (int l = 0; l < d->depth; ++l) {
    const vcap_vit_layer& ly = d->layers[l];
    // The last block feeds only the class-token rows (final LN on CLS rows, CLS temporal pool:
    // video_encoder.py:256-258, pool="cls" at caption_model.py:45), so after its QKV projection
    // (K/V of every token are needed) it runs on the BT CLS rows only: CLS-query attention into a
    // compact [BT, D] buffer, then attn-proj / LN2 / fc1 / fc2 on BT rows with the residual rows
    // remapped to x[bt*N] (GemmEpi G = 1, Gs = N).  Outputs are identical; 6 % fewer FLOPs.
    const bool last = l == d->depth - 1;
    const int Mt = last ? BT : M;                       // rows after the QKV projection
    const int slot = snap ? l - (d->depth - snap->n_tail) : -1;   // >= 0: a block whose activations are kept
    if (slot >= 0) {
      const size_t ea = esize(adt), n = (size_t)M * D;
      VCAP_TRY(hipMemcpyAsync(snap->x0 + slot * n, w.x, n * 4, hipMemcpyDeviceToDevice, s), "snapshot x0");
      w.qkv = snap->qkv + slot * 3 * n * ea;
      w.attn = snap->attn + slot * n * ea;
      w.act = snap->act + (size_t)slot * M * d->mlp * ea;
    }
    const std::string probe_attn = vit_site("attention", last);
    // MXFP8 mode, per GEMM (weight scales present): the producer of its A operand emits MXFP8
    const bool mq = mx && ly.qkv_ws, mp = mx && ly.proj_ws, m1 = mx && ly.fc1_ws, m2 = mx && ly.fc2_ws;
    const int dq = mq ? VCAP_DT_MXFP8 : adt, dp = mp ? VCAP_DT_MXFP8 : adt;
    const int d1 = m1 ? VCAP_DT_MXFP8 : adt, d2 = m2 ? VCAP_DT_MXFP8 : adt;
    if (int rc = norm(mq, D, ly.ln1_g, ly.ln1_b, M, "norm1")) return rc;
    GemmEpi e1{ly.qkv_b, nullptr, 0, 0, 0, 0, 0, 0, 0, mq ? w.xn_s : nullptr, mq ? ly.qkv_ws : nullptr, nullptr};
    if (slot < 0 && vit_layer_fused(d, ly)) {
      // QKV projection + attention in one kernel: q / k / v stay on chip
      ProbeScope ps(probe_attn.c_str(), s, M);
      VCAP_TRY(vcap_vit_qkv_attention_dispatch(adt, w.xn, ly.qkv_w, ly.qkv_b, w.attn, BT, N, d->heads, last, s),
               "qkv_attention");
    } else {
      {
        ProbeScope ps("vit.qkv", s, M);
        VCAP_TRY(vcap_gemm_dispatch(dq, adt, w.xn, D, ly.qkv_w, D, w.qkv, 3 * D, M, 3 * D, D, e1, s), "qkv");
      }
      ProbeScope ps(probe_attn.c_str(), s, M);
      if (mp)
        VCAP_TRY(vcap_vit_attention_mx_dispatch(w.qkv, w.attn, w.xn_s, BT, N, d->heads, s, last), "attention");
      else
        VCAP_TRY(vcap_vit_attention_dispatch(adt, w.qkv, w.attn, BT, N, d->heads, s, last), "attention");
    }
    // MXFP8: the attention output arrives as MXFP8 (its scales reuse xn_s, free until norm2)
    GemmEpi e2{ly.proj_b, w.x, D, 0, 1, last ? 1 : 0, last ? N : 0, 0, 0, mp ? w.xn_s : nullptr,
               mp ? ly.proj_ws : nullptr, nullptr, last ? w.splitk : nullptr, w.splitk_bytes};
    {
      ProbeScope ps(vit_site("proj", last).c_str(), s, Mt);
      VCAP_TRY(vcap_gemm_dispatch(dp, VCAP_DT_F32, w.attn, D, ly.proj_w, D, w.x, D, Mt, D, D, e2, s), "attn_proj");
    }
    if (slot >= 0) {   // the stream after the attention residual (the last block: its BT class-token rows)
      float* x1 = snap->x1 + (size_t)slot * M * D;
      if (last)
        VCAP_TRY(vcap_vit_rows_copy_dispatch(w.x, (long)N * D, x1, D, BT, D, s), "snapshot x1");
      else
        VCAP_TRY(hipMemcpyAsync(x1, w.x, (size_t)M * D * 4, hipMemcpyDeviceToDevice, s), "snapshot x1");
    }
    // CLS rows of x are N*D apart
    if (int rc = norm(m1, last ? (long)N * D : D, ly.ln2_g, ly.ln2_b, Mt, "norm2")) return rc;
    // fc1 emits MXFP8 straight from its epilogue when both MLP GEMMs are MXFP8; an MXFP8 fc2 after
    // a bf16 fc1 quantises the bf16 activation (vcap_mx_quantize) into the free qkv buffer
    const bool fused_q = m1 && m2;
    GemmEpi e3{ly.fc1_b, nullptr, 0, 1, 0, 0, 0, 0, 0, m1 ? w.xn_s : nullptr, m1 ? ly.fc1_ws : nullptr,
               fused_q ? w.act_s : nullptr};
    {
      ProbeScope ps(vit_site("fc1", last).c_str(), s, Mt);
      VCAP_TRY(vcap_gemm_dispatch(d1, fused_q ? VCAP_DT_MXFP8 : adt, w.xn, D, ly.fc1_w, D, w.act, d->mlp, Mt, d->mlp,
                                  D, e3, s),
               "fc1");
    }
    const void* a2 = w.act;
    if (m2 && !fused_q) {
      VCAP_TRY(vcap_mx_quantize_dispatch(adt, w.act, d->mlp, Mt, d->mlp, (uint8_t*)w.qkv, w.act_s, Mt, s), "fc1 quant");
      a2 = w.qkv;
    }
    GemmEpi e4{ly.fc2_b, w.x, D, 0, 1, last ? 1 : 0, last ? N : 0, 0, 0, m2 ? w.act_s : nullptr,
               m2 ? ly.fc2_ws : nullptr, nullptr, last ? w.splitk : nullptr, w.splitk_bytes};
    {
      ProbeScope ps(vit_site("fc2", last).c_str(), s, Mt);
      VCAP_TRY(vcap_gemm_dispatch(d2, VCAP_DT_F32, a2, d->mlp, ly.fc2_w, d->mlp, w.x, D, Mt, D, d->mlp, e4, s),
               "fc2");
    }
  }
  const float ls = pd ? pd->ln_scale : 0.f, iw = pd ? pd->in_weight : 0.f;
  const int MO = pd ? pd->prefix_len * pd->n_embd : 0;
  VCAP_TRY(vcap_vit_head_prefix_dispatch(w.x, B, T, N, D, d->norm_g, d->norm_b, d->ln_eps, d->proj_w, d->proj_b,
                                         d->video_dim, ls, iw, pd ? pd->mapper_w : nullptr,
                                         pd ? pd->mapper_b : nullptr, MO, enc_out, prefix_out, nullptr,
                                         (float*)w.xn, s, dt == VCAP_DT_F16),
           "head_prefix");
  if (snap) {
    snap->x = w.x;
    snap->xn = w.xn;
    snap->patches = patches;
  }
  return 0;
}
