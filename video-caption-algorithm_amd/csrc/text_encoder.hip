// Text tower of the alignment model: the pieces ViTTextAlignModel.encode_text
// (src/models/vit_text_align.py:67-79) needs beside the rows-packed GEMVs of decode.hip.
//
//   x = txt_emb[ids]                                             vcap_text_gather_kernel
//   per nn.TransformerEncoderLayer (post-LN, ReLU, batch_first, no mask of any kind):
//     qkv = in_proj(x)            rows GEMV, PRO_DIRECT + EPI_STORE -> T [M, 3E]
//     a   = softmax(q k^T / 8) v  vcap_text_attention_kernel
//     x   = LN1(x + out_proj(a))  rows GEMV EPI_RESID (x += ...), then vcap_text_resid_ln_kernel
//     x   = LN2(x + linear2(relu(linear1(x))))   EPI_RELU, EPI_RESID, vcap_text_resid_ln_kernel
//   out = normalize(txt_proj(masked mean over ids != pad))      vcap_text_pool_kernel
//
// M = B*L rows, E = 64 H features, L <= 64.  The residual stream x, LayerNorm, the softmax, the pool,
// the projection and the normalisation are f32 whatever the operand dtype T (f32 / bf16) is; T holds
// the GEMV operands, the stored q/k/v, the attention output and the ReLU output.
//
// The attention is plain VALU, not MFMA: one (caption, head) is at most a 64 x 64 x 64 score tile and
// as much again for P.V, 0.5 MFLOP - the launch, not the arithmetic, is what it costs - and on the VALU
// the f32 path is one exact fma chain per score with no fragment shuffles between Q.K^T, the softmax and
// P.V.  One lane owns one key (its K row in 64 registers) and one output feature (its V column in 64
// registers); the query row and the probabilities reach the lanes as v_readlane broadcasts, so a wave
// uses no LDS and meets no barrier.  Every reduction has a fixed order; nothing is accumulated atomically.
#include "vcap_common.h"
#include "vcap_kernels.h"

namespace {

VCAP_DEV float lane_bcast(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// four T starting at a 4-element boundary <- f32x4
VCAP_DEV void store4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
VCAP_DEV void store4(bf16_t* p, f32x4 v) {
  *reinterpret_cast<u32x2*>(p) = (u32x2){pack_bf2(v.x, v.y), pack_bf2(v.z, v.w)};
}
VCAP_DEV void store2(float* p, f32x2 v) { *reinterpret_cast<f32x2*>(p) = v; }
VCAP_DEV void store2(bf16_t* p, f32x2 v) { *reinterpret_cast<uint32_t*>(p) = pack_bf2(v.x, v.y); }

}  // namespace

// ------------------------------------------------------------------------------------------------
// Token gather: row m of x (f32) and xt (T) = emb[ids[m]].  The pad row is read as stored.  An id outside
// [0, vocab) reads nothing: its row is NaN, which the encoder spreads over that caption alone (attention
// and the pool never cross captions, and a GEMV row depends on its own activation row only).
template <typename T>
__global__ __launch_bounds__(256) void vcap_text_gather_kernel(const int* __restrict__ ids,
                                                               const float* __restrict__ emb, int vocab, int E,
                                                               float* __restrict__ x, T* __restrict__ xt) {
  const int m = blockIdx.x;
  const int id = ids[m];
  const bool ok = (unsigned)id < (unsigned)vocab;
  const float* src = emb + (long)(ok ? id : 0) * E;
  const float nan = __int_as_float(0x7FC00000);
  for (int c = threadIdx.x * 4; c < E; c += 1024) {
    f32x4 v = *reinterpret_cast<const f32x4*>(src + c);
    if (!ok) v = (f32x4){nan, nan, nan, nan};
    store4(x + (long)m * E + c, v);
    store4(xt + (long)m * E + c, v);
  }
}

// ------------------------------------------------------------------------------------------------
// Bidirectional attention of one (caption, head) per workgroup; wave w takes the queries w, w + 4, ...
// qkv [B*L, 3E] as in_proj stored it (q | k | v, head h at columns 64 h), out [B*L, E].  No mask: pad
// positions are ordinary keys and queries, as in the reference, which passes no key-padding mask.
// Score of (query i, key j) = sum over d = 0..63 in order of (q[i][d] / 8) * k[j][d] (the 1/8 is exact),
// p = exp(s - max) / sum over the wave's fixed tree, out[i][d] = sum over j = 0..63 in order of
// p[j] * v[j][d]; lanes >= L hold p = 0 and v = 0.
template <typename T>
__global__ __launch_bounds__(256) void vcap_text_attention_kernel(const T* __restrict__ qkv, T* __restrict__ out, int L,
                                                                  int H) {
  constexpr int EL = Frag<T>::kElems;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int E = H * 64;
  const long ld = 3L * E;
  const T* base = qkv + (long)b * L * ld + h * 64;

  float kr[64], vc[64];
  {
    const T* kp = base + (long)min(lane, L - 1) * ld + E;  // clamped: lanes >= L are discarded below
#pragma unroll
    for (int c = 0; c < 64 / EL; ++c) {
      const u32x4 raw = *reinterpret_cast<const u32x4*>(kp + c * EL);
      if constexpr (sizeof(T) == 4) {
        kr[c * 4 + 0] = __uint_as_float(raw.x);
        kr[c * 4 + 1] = __uint_as_float(raw.y);
        kr[c * 4 + 2] = __uint_as_float(raw.z);
        kr[c * 4 + 3] = __uint_as_float(raw.w);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          kr[c * 8 + 2 * r] = __uint_as_float(raw[r] << 16);
          kr[c * 8 + 2 * r + 1] = __uint_as_float(raw[r] & 0xFFFF0000u);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 64; ++j) {
    const float v = Num<T>::to_f(base[(long)min(j, L - 1) * ld + 2 * E + lane]);
    vc[j] = j < L ? v : 0.f;
  }

  for (int i = wave; i < L; i += 4) {
    const float qv = Num<T>::to_f(base[(long)i * ld + lane]) * 0.125f;
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < 64; ++d) s = fmaf(lane_bcast(qv, d), kr[d], s);
    s = lane < L ? s : -INFINITY;
    const float mx = wave_max(s);
    float p = expf(s - mx);
    p = p / wave_sum(p);
    float o = 0.f;
#pragma unroll
    for (int j = 0; j < 64; ++j) o = fmaf(lane_bcast(p, j), vc[j], o);
    out[((long)b * L + i) * E + h * 64 + lane] = Num<T>::from_f(o);
  }
}

// ------------------------------------------------------------------------------------------------
// Residual LayerNorm: x <- LN(x) in place on the f32 stream (the residual GEMV before it did x += ...),
// and the T copy the next GEMV reads.  One wave per row, the row in registers: E % 128 == 0, E <= 1024,
// lane l holds features [128 c + 2 l, +2) of chunk c.  Two-pass mean / variance, sums per lane in chunk
// order, then the wave's tree.
template <typename T>
__global__ __launch_bounds__(256) void vcap_text_resid_ln_kernel(float* __restrict__ x, T* __restrict__ xt,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, int M, int E,
                                                                 float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int nc = E / 128;
  float* xr = x + (long)row * E;
  f32x2 v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = *reinterpret_cast<const f32x2*>(xr + min(c, nc - 1) * 128 + lane * 2);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c)
    if (c < nc) s += v[c].x + v[c].y;
  const float mean = wave_sum(s) / (float)E;
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c)
    if (c < nc) {
      v[c] = v[c] - mean;
      ss = fmaf(v[c].x, v[c].x, fmaf(v[c].y, v[c].y, ss));
    }
  const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)E + eps);
#pragma unroll
  for (int c = 0; c < 8; ++c)
    if (c < nc) {
      const int f = c * 128 + lane * 2;
      const f32x2 g = *reinterpret_cast<const f32x2*>(gamma + f), bb = *reinterpret_cast<const f32x2*>(beta + f);
      const f32x2 y = __builtin_elementwise_fma(v[c] * rstd, g, bb);
      store2(xr + f, y);
      store2(xt + (long)row * E + f, y);
    }
}

// ------------------------------------------------------------------------------------------------
// Pool, project, normalise: one workgroup of 16 waves per caption.
//   pooled[e] = (sum over l = 0..L-1 in order of x[l][e] * (ids[l] != pad)) / max(count, 1)
//   y[p]      = (sum over e of w[p][e] * pooled[e]: per lane chunks in order, then the wave's tree) + bias[p]
//   out[p]    = y[p] / max(sqrt(sum over p of y[p]^2), 1e-12): per lane p = l, l + 64, ... in order, then the tree
// An all-pad caption pools to zeros and comes out as normalize(bias).
__global__ __launch_bounds__(1024) void vcap_text_pool_kernel(const float* __restrict__ x, const int* __restrict__ ids,
                                                              int pad_id, int L, int E, const float* __restrict__ pw,
                                                              const float* __restrict__ pb, int P,
                                                              float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float pooled[1024];
  __shared__ float yv[1024];
  __shared__ float keep[64];
  __shared__ float s_norm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const float* xb = x + (long)b * L * E;
  const int* idb = ids + (long)b * L;
  if (tid < 64) keep[tid] = (tid < L && idb[tid] != pad_id) ? 1.f : 0.f;
  __syncthreads();
  if (tid < E) {
    float cnt = 0.f, acc = 0.f;
#pragma unroll 8
    for (int l = 0; l < L; ++l) {
      acc = fmaf(xb[(long)l * E + tid], keep[l], acc);
      cnt += keep[l];
    }
    pooled[tid] = acc / fmaxf(cnt, 1.f);
  }
  __syncthreads();
  const int nc = E / 128, per_wave = P / 16;  // P % 64 == 0: a multiple of 4 outputs per wave
  for (int k = 0; k < per_wave; k += 4) {
    f32x2 w[4][8];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int c = 0; c < 8; ++c)
        w[u][c] = *reinterpret_cast<const f32x2*>(pw + (long)(wave * per_wave + k + u) * E + min(c, nc - 1) * 128 +
                                                  lane * 2);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (c < nc) {
          const f32x2 pv = *reinterpret_cast<const f32x2*>(pooled + c * 128 + lane * 2);
          acc = fmaf(w[u][c].x, pv.x, fmaf(w[u][c].y, pv.y, acc));
        }
      acc = wave_sum(acc);
      const int p = wave * per_wave + k + u;
      if (lane == 0) yv[p] = acc + pb[p];
    }
  }
  __syncthreads();
  if (wave == 0) {
    float ss = 0.f;
    for (int p = lane; p < P; p += 64) ss = fmaf(yv[p], yv[p], ss);
    ss = wave_sum(ss);
    if (lane == 0) s_norm = fmaxf(sqrtf(ss), 1e-12f);
  }
  __syncthreads();
  if (tid < P) out[(long)b * P + tid] = yv[tid] / s_norm;
}

// ------------------------------------------------------------------------------------------------
hipError_t vcap_text_gather_dispatch(int dt, const int* ids, int M, const float* emb, int vocab, int E, float* x,
                                     void* xt, hipStream_t s) {
  if (M <= 0 || E <= 0 || E % 4 || vocab <= 0) return hipErrorInvalidValue;
  if (dt == VCAP_DT_BF16)
    hipLaunchKernelGGL((vcap_text_gather_kernel<bf16_t>), dim3(M), dim3(256), 0, s, ids, emb, vocab, E, x, (bf16_t*)xt);
  else if (dt == VCAP_DT_F32)
    hipLaunchKernelGGL((vcap_text_gather_kernel<float>), dim3(M), dim3(256), 0, s, ids, emb, vocab, E, x, (float*)xt);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t vcap_text_attention_dispatch(int dt, const void* qkv, void* out, int B, int L, int H, hipStream_t s) {
  if (B <= 0 || H <= 0 || L < 1 || L > 64) return hipErrorInvalidValue;
  if (dt == VCAP_DT_BF16)
    hipLaunchKernelGGL((vcap_text_attention_kernel<bf16_t>), dim3(B * H), dim3(256), 0, s, (const bf16_t*)qkv,
                       (bf16_t*)out, L, H);
  else if (dt == VCAP_DT_F32)
    hipLaunchKernelGGL((vcap_text_attention_kernel<float>), dim3(B * H), dim3(256), 0, s, (const float*)qkv,
                       (float*)out, L, H);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t vcap_text_resid_ln_dispatch(int dt, float* x, void* xt, const float* gamma, const float* beta, int M, int E,
                                       float eps, hipStream_t s) {
  if (M <= 0 || E <= 0 || E % 128 || E > 1024) return hipErrorInvalidValue;
  const dim3 grid((M + 3) / 4);
  if (dt == VCAP_DT_BF16)
    hipLaunchKernelGGL((vcap_text_resid_ln_kernel<bf16_t>), grid, dim3(256), 0, s, x, (bf16_t*)xt, gamma, beta, M, E,
                       eps);
  else if (dt == VCAP_DT_F32)
    hipLaunchKernelGGL((vcap_text_resid_ln_kernel<float>), grid, dim3(256), 0, s, x, (float*)xt, gamma, beta, M, E, eps);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t vcap_text_pool_dispatch(const float* x, const int* ids, int pad_id, int B, int L, int E, const float* pw,
                                   const float* pb, int P, float* out, hipStream_t s) {
  if (B <= 0 || L < 1 || L > 64 || E <= 0 || E % 128 || E > 1024 || P < 64 || P % 64 || P > 1024)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(vcap_text_pool_kernel, dim3(B), dim3(1024), 0, s, x, ids, pad_id, L, E, pw, pb, P, out);
  return hipGetLastError();
}
