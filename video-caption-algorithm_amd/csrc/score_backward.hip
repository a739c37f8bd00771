// Kernels of vcap_gpt2_score_backward (schedule: runtime_gpt2_grad.hip): the gradient of the
// teacher-forced target log-probs with respect to inputs_embeds through GPT-2 - the activation gradients.
// (The weight gradients of vcap_gpt2_score_backward_tail's unfrozen blocks are side outputs of the same
// walk: the products in gpt2_weight_grad.hip, the column sums in text_backward.hip, and the STATS form of
// vcap_ln_backward_kernel below.)
//
//   vcap_grad_gemm_kernel       C[m][n] = sum_k A[m][k] W[n][k] with the 128x128 MFMA tile loop of
//                               gemm_tile.h, operands in the decoder dtype T, f32 accumulation and f32
//                               output.  One kernel at every M (no policy, no M-dependent split), so a
//                               row's bits do not depend on the other rows of the launch.  blockIdx.z
//                               takes a fixed K range (a constant number of columns: 256 in the block
//                               products, 2048 in the K = V product of the lm_head backward - these GEMMs
//                               have 2 to 48 output tiles, far fewer than CUs) and writes its own f32 slab;
//                               vcap_grad_slab_sum_kernel adds the slabs in slab order, then the bias.
//   vcap_score_lse_kernel       a row's log-sum-exp from the score kernel's (max, sum exp) parts, merged
//                               exactly as vcap_score_combine_kernel merges them
//   vcap_score_dlogit_kernel    dlogit[m][v] = w[m] (1[v == t_m] - exp(logit[m][v] - lse[m])) in T; rows that
//                               are not counted and columns past V are written as +0 and cost no exp
//   vcap_ln_backward_kernel     g[m] += dLN(x[m]) . dy[m]: one row per wave, the row in registers (E <= 1024),
//                               mean and rstd recomputed from the snapshot x; <true> also stores them per row
//                               (an unfrozen layer's gamma / beta column sums read them), same arithmetic for g
//   vcap_gelu_backward_kernel   du = dact * gelu_new'(u), the derivative of the sigmoid form of gelu_tanh
//   vcap_attn_bwd_rows_kernel   one wave per (sequence, head, query i): P[i][:], dP = dO_i . V^T, delta_i =
//                               sum_j P dP, dS = P (dP - delta) / 8 -> the P and dS rows of the call's scratch
//   vcap_attn_bwd_sums_kernel   one wave per (sequence, head, position r), lane = head dimension:
//                               dq_r = sum_{j<=r} dS[r][j] k_j, dk_r = sum_{i>=r} dS[i][r] q_i,
//                               dv_r = sum_{i>=r} P[i][r] dO_i, each in index order by ONE wave: no sums
//                               across waves or workgroups, no atomics.  A hidden key's P and dS are
//                               exactly 0.
//   vcap_grad_finish_kernel     grad_embeds = g + 0 (wpe is added to the embeddings, so the gradient passes
//                               through unchanged); every row of a sequence whose first key is hidden is NaN
//
// Rounding points with a bf16 decoder (f32 decoders round nowhere): the operands of every MFMA product
// are bf16 (RNE) - the recomputed LayerNorm rows, dlogit, the residual gradient where it enters the
// c_proj^T products, du = dact * gelu'(u), and dq | dk | dv - and the recomputed q, k, v are rounded to
// bf16 values as the forward stores them.  Accumulation, the residual gradient stream, the softmax,
// LayerNorm and GELU backward arithmetic are f32.
//
// Exact zeros: a row whose incoming gradient is all zero leaves every kernel as +0 - accumulators start
// at +0 and only add (+0 + -0 = +0), dlogit and the hidden keys' dS are written as literal zeros, and the
// residual gradient is only ever added to.
#include "gemm_tile.h"
#include "vcap_common.h"
#include "vcap_kernels.h"

using namespace gemm_tile;

template <typename T>
__global__ __launch_bounds__(256) void vcap_grad_gemm_kernel(const T* __restrict__ A, long lda,
                                                             const T* __restrict__ W, long ldw,
                                                             float* __restrict__ C, long ldc, long slab, int M, int N,
                                                             int nkt, int kt_per) {
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, fr = lane & 15, fg = lane >> 4;
  const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM;
  const int kt0 = blockIdx.z * kt_per;
  const int nk = min(kt_per, nkt - kt0);
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  tile_loop(A, lda, W, ldw, m0, M, n0, N, kt0, nk, smem, acc);
  float* out = C + (long)blockIdx.z * slab;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm * 64 + i * 16 + fr;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = n0 + wn * 64 + j * 16 + 4 * fg;  // N % 128 == 0: no column edge
      *reinterpret_cast<f32x4*>(out + (long)m * ldc + col) = acc[i][j];
    }
  }
}

// out[i] = slab 0 [i] + slab 1 [i] + ... in slab order (n4 float4 per slab), then + bias[column] and the
// rounding to bf16 values of the recomputed q | k | v (rows of N columns)
__global__ __launch_bounds__(256) void vcap_grad_slab_sum_kernel(const f32x4* __restrict__ slabs, long n4, int nslab,
                                                                 const float* __restrict__ bias, int N, int round_bf16,
                                                                 f32x4* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  f32x4 s = slabs[i];
  for (int z = 1; z < nslab; ++z) s += slabs[(long)z * n4 + i];
  if (bias) s += *reinterpret_cast<const f32x4*>(bias + (i * 4) % N);
  if (round_bf16) {
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = bf2f(f2bf(s[e]));
  }
  out[i] = s;
}

// One wave per row: the parts merged in vcap_score_combine_kernel's order -> lse = max + log(sum)
__global__ __launch_bounds__(256) void vcap_score_lse_kernel(const float* __restrict__ part_max,
                                                             const float* __restrict__ part_sum, int nparts, int M,
                                                             float* __restrict__ lse) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  float mx = -INFINITY, sum = 0.f;
  for (int p = lane; p < nparts; p += 64) {
    const float pm = part_max[(long)row * nparts + p], ps = part_sum[(long)row * nparts + p];
    if (pm > mx) {
      sum = sum * expf(mx - pm) + ps;
      mx = pm;
    } else if (pm != -INFINITY) {
      sum += ps * expf(pm - mx);
    }
  }
  const float gm = wave_max(mx);
  const float tot = wave_sum(mx == -INFINITY ? 0.f : sum * expf(mx - gm));
  if (lane == 0) lse[row] = gm + logf(tot);
}

// grid (Vpad / 128, M), 128 threads: one column each
template <typename T>
__global__ __launch_bounds__(128) void vcap_score_dlogit_kernel(const float* __restrict__ logits,
                                                                const float* __restrict__ lse,
                                                                const int* __restrict__ targets,
                                                                const float* __restrict__ w, int V, int Vpad,
                                                                T* __restrict__ dl) {
  const int m = blockIdx.y;
  const int v = blockIdx.x * 128 + threadIdx.x;
  const int t = targets[m];
  float d = 0.f;
  if (t >= 0 && t < V && v < V) {
    const float wv = w ? w[m] : -1.f;
    d = wv * ((v == t ? 1.f : 0.f) - expf(logits[(long)m * V + v] - lse[m]));
  }
  dl[(long)m * Vpad + v] = Num<T>::from_f(d);
}

// g[m][:] += rstd (dyh - mean(dyh) - xh mean(dyh xh)), dyh = dy gamma, xh = (x - mean) rstd.  One row
// per wave, lane l holds columns 128 k + 2 l + {0, 1}, k < E / 128 <= 8.  STATS (the tail call's unfrozen
// layers): the row's (mean, rstd) also go to stats[m] for the gamma / beta column sums; g's arithmetic is
// the same.
template <bool STATS>
__global__ __launch_bounds__(256) void vcap_ln_backward_kernel(const float* __restrict__ x,
                                                               const float* __restrict__ dy,
                                                               const float* __restrict__ gamma, float eps, int M,
                                                               int E, float* __restrict__ g,
                                                               float* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int nk = E >> 7;
  const float inv = 1.0f / (float)E;
  f32x2 xv[8], dv[8];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    xv[k] = (f32x2){0.f, 0.f};
    dv[k] = (f32x2){0.f, 0.f};
    if (k < nk) {
      const long o = (long)row * E + k * 128 + 2 * lane;
      xv[k] = *reinterpret_cast<const f32x2*>(x + o);
      const f32x2 gm = *reinterpret_cast<const f32x2*>(gamma + k * 128 + 2 * lane);
      dv[k] = *reinterpret_cast<const f32x2*>(dy + o) * gm;
      s += xv[k].x + xv[k].y;
    }
  }
  const float mean = wave_sum(s) * inv;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (k < nk) {
      xv[k] = xv[k] - mean;
      q += fmaf(xv[k].x, xv[k].x, xv[k].y * xv[k].y);
    }
  const float rstd = 1.0f / sqrtf(wave_sum(q) * inv + eps);
  if constexpr (STATS) {
    if (lane == 0) *reinterpret_cast<f32x2*>(stats + 2L * row) = (f32x2){mean, rstd};
  }
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (k < nk) {
      xv[k] = xv[k] * rstd;  // xh
      s1 += dv[k].x + dv[k].y;
      s2 += fmaf(dv[k].x, xv[k].x, dv[k].y * xv[k].y);
    }
  const float m1 = wave_sum(s1) * inv, m2 = wave_sum(s2) * inv;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (k < nk) {
      const long o = (long)row * E + k * 128 + 2 * lane;
      f32x2 gv = *reinterpret_cast<f32x2*>(g + o);
      gv.x += rstd * (dv[k].x - m1 - xv[k].x * m2);
      gv.y += rstd * (dv[k].y - m1 - xv[k].y * m2);
      *reinterpret_cast<f32x2*>(g + o) = gv;
    }
}

// gelu_new(x) = x sig(z), z = 2 c (x + 0.044715 x^3), c = sqrt(2 / pi) (vcap_common.h gelu_tanh):
// gelu' = sig + x sig (1 - sig) 2 c (1 + 3 * 0.044715 x^2)
VCAP_DEV float gelu_new_grad(float x) {
  const float c2 = 2.0f * 0.7978845608028654f;
  const float z = c2 * x * fmaf(0.044715f, x * x, 1.0f);
  const float sg = 1.0f / (1.0f + expf(-z));
  const float dz = c2 * fmaf(3.0f * 0.044715f, x * x, 1.0f);
  return sg + x * sg * (1.0f - sg) * dz;
}

template <typename T>
__global__ __launch_bounds__(256) void vcap_gelu_backward_kernel(const float* __restrict__ u,
                                                                 const float* __restrict__ dact, long n,
                                                                 T* __restrict__ du) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) du[i] = Num<T>::from_f(dact[i] * gelu_new_grad(u[i]));
}

__global__ __launch_bounds__(256) void vcap_grad_to_bf16_kernel(const float* __restrict__ x, long n,
                                                                bf16_t* __restrict__ y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = f2bf(x[i]);
}

// grid (ceil(S / 4), B * H): wave -> query i; lane -> keys lane + 64 t, t < 8 (S <= 512).
// qkv [B*S][3E] f32 (q | k | v), dO [B*S][E] f32; P, dS: [B*H][S][S] f32 scratch, columns j <= i written.
__global__ __launch_bounds__(256) void vcap_attn_bwd_rows_kernel(const float* __restrict__ qkv,
                                                                 const float* __restrict__ dO,
                                                                 const uint8_t* __restrict__ kmask, int S, int H,
                                                                 float* __restrict__ P, float* __restrict__ dS) {
  __shared__ __attribute__((aligned(16))) float s_q[4][64];
  __shared__ __attribute__((aligned(16))) float s_do[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;
  const int b = blockIdx.y / H, h = blockIdx.y % H;
  const int E = H * 64;
  const bool live = i < S;
  const int ic = live ? i : S - 1;
  const long row = (long)b * S + ic;
  s_q[wave][lane] = qkv[row * 3 * E + h * 64 + lane];
  s_do[wave][lane] = dO[row * E + h * 64 + lane];
  __syncthreads();
  if (!live) return;
  float sc[8], dp[8];
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    sc[t] = -INFINITY;
    dp[t] = 0.f;
    if (t * 64 > i) continue;  // wave-uniform
    const int j = t * 64 + lane;
    const bool ok = j <= i && (!kmask || kmask[(long)b * S + j] != 0);
    const int jc = j <= i ? j : i;
    const float* kr = qkv + ((long)b * S + jc) * 3 * E + E + h * 64;
    const float* vr = kr + E;
    float a = 0.f, c = 0.f;
#pragma unroll
    for (int d = 0; d < 64; d += 4) {
      const f32x4 kv = *reinterpret_cast<const f32x4*>(kr + d);
      const f32x4 vv = *reinterpret_cast<const f32x4*>(vr + d);
      const f32x4 qv = *reinterpret_cast<const f32x4*>(&s_q[wave][d]);
      const f32x4 ov = *reinterpret_cast<const f32x4*>(&s_do[wave][d]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        a = fmaf(qv[e], kv[e], a);
        c = fmaf(ov[e], vv[e], c);
      }
    }
    if (ok) {
      sc[t] = a * 0.125f;
      dp[t] = c;
      mx = fmaxf(mx, sc[t]);
    }
  }
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    sc[t] = sc[t] == -INFINITY ? 0.f : expf(sc[t] - mx);  // a hidden or future key: exactly 0
    sum += sc[t];
  }
  const float rs = 1.0f / wave_sum(sum);
  float dl = 0.f;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    sc[t] *= rs;
    dl = fmaf(sc[t], dp[t], dl);
  }
  dl = wave_sum(dl);
  const long base = ((long)blockIdx.y * S + i) * S;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int j = t * 64 + lane;
    if (j <= i) {
      P[base + j] = sc[t];
      dS[base + j] = sc[t] == 0.f ? 0.f : sc[t] * (dp[t] - dl) * 0.125f;
    }
  }
}

// grid (ceil(S / 4), B * H): wave -> position r, lane -> head dimension d.  dqkv [B*S][3E] in T.
template <typename T>
__global__ __launch_bounds__(256) void vcap_attn_bwd_sums_kernel(const float* __restrict__ qkv,
                                                                 const float* __restrict__ dO,
                                                                 const float* __restrict__ P,
                                                                 const float* __restrict__ dS, int S, int H,
                                                                 T* __restrict__ dqkv) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= S) return;
  const int b = blockIdx.y / H, h = blockIdx.y % H;
  const int E = H * 64;
  const float* q0 = qkv + (long)b * S * 3 * E + h * 64 + lane;  // + row * 3E
  const float* o0 = dO + (long)b * S * E + h * 64 + lane;
  const float* Pb = P + (long)blockIdx.y * S * S;
  const float* Sb = dS + (long)blockIdx.y * S * S;
  float dq = 0.f, dk = 0.f, dv = 0.f;
  for (int j = 0; j <= r; ++j) dq = fmaf(Sb[(long)r * S + j], q0[(long)j * 3 * E + E], dq);
  for (int i = r; i < S; ++i) {
    dk = fmaf(Sb[(long)i * S + r], q0[(long)i * 3 * E], dk);
    dv = fmaf(Pb[(long)i * S + r], o0[(long)i * E], dv);
  }
  T* out = dqkv + ((long)b * S + r) * 3 * E + h * 64 + lane;
  out[0] = Num<T>::from_f(dq);
  out[E] = Num<T>::from_f(dk);
  out[2 * E] = Num<T>::from_f(dv);
}

__global__ __launch_bounds__(256) void vcap_grad_finish_kernel(const float* __restrict__ g,
                                                               const uint8_t* __restrict__ kmask, int S, int E, long n,
                                                               float* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long seq = i / ((long)S * E);
  const bool bad = kmask && kmask[seq * S] == 0;
  out[i] = bad ? __builtin_nanf("") : g[i] + 0.f;  // + 0: a -0 cannot leave
}

// ---- dispatchers ------------------------------------------------------------------------------------
int vcap_grad_bk(int dt) { return ROWB / (int)vcap_dt_size(dt); }

hipError_t vcap_grad_gemm_dispatch(int dt, const void* A, long lda, const void* W, long ldw, float* C, long ldc,
                                   int M, int N, int K, int k_per_slab, hipStream_t s) {
  if (dt != VCAP_DT_F32 && dt != VCAP_DT_BF16) return hipErrorInvalidValue;
  const int bk = vcap_grad_bk(dt);
  if (M <= 0 || N <= 0 || N % BN || K <= 0 || K % bk || (k_per_slab && k_per_slab % bk) ||
      ((uintptr_t)A & 15) || ((uintptr_t)W & 15) || ((uintptr_t)C & 15) || (lda * (long)vcap_dt_size(dt)) % 16 ||
      (ldw * (long)vcap_dt_size(dt)) % 16 || ldc % 4)
    return hipErrorInvalidValue;
  const int nkt = K / bk;
  const int kt_per = k_per_slab ? k_per_slab / bk : nkt;
  const dim3 grid(N / BN, (M + BM - 1) / BM, (nkt + kt_per - 1) / kt_per), block(256);
  const long slab = (long)M * ldc;
  if (dt == VCAP_DT_BF16)
    hipLaunchKernelGGL(vcap_grad_gemm_kernel<bf16_t>, grid, block, 0, s, (const bf16_t*)A, lda, (const bf16_t*)W, ldw,
                       C, ldc, slab, M, N, nkt, kt_per);
  else
    hipLaunchKernelGGL(vcap_grad_gemm_kernel<float>, grid, block, 0, s, (const float*)A, lda, (const float*)W, ldw, C,
                       ldc, slab, M, N, nkt, kt_per);
  return hipGetLastError();
}

hipError_t vcap_grad_slab_sum_dispatch(const float* slabs, long n, int nslab, const float* bias, int N,
                                       int round_bf16, float* out, hipStream_t s) {
  if (n <= 0 || N <= 0 || N % 4 || n % N || nslab <= 0 || ((uintptr_t)bias & 15)) return hipErrorInvalidValue;
  const long n4 = n / 4;
  hipLaunchKernelGGL(vcap_grad_slab_sum_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s,
                     (const f32x4*)slabs, n4, nslab, bias, N, round_bf16, (f32x4*)out);
  return hipGetLastError();
}

hipError_t vcap_score_dlogit_dispatch(int dt, const float* part_max, const float* part_sum, int nparts,
                                      const float* logits, const int* targets, const float* w, int M, int V, int Vpad,
                                      float* lse, void* dl, hipStream_t s) {
  if (M <= 0 || V <= 0 || Vpad < V || Vpad % 128) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vcap_score_lse_kernel, dim3((M + 3) / 4), dim3(256), 0, s, part_max, part_sum, nparts, M, lse);
  if (hipError_t e = hipGetLastError()) return e;
  const dim3 grid(Vpad / 128, M), block(128);
  if (dt == VCAP_DT_BF16)
    hipLaunchKernelGGL(vcap_score_dlogit_kernel<bf16_t>, grid, block, 0, s, logits, (const float*)lse, targets, w, V,
                       Vpad, (bf16_t*)dl);
  else if (dt == VCAP_DT_F32)
    hipLaunchKernelGGL(vcap_score_dlogit_kernel<float>, grid, block, 0, s, logits, (const float*)lse, targets, w, V,
                       Vpad, (float*)dl);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t vcap_ln_backward_dispatch(const float* x, const float* dy, const float* gamma, float eps, int M, int E,
                                     float* g, hipStream_t s) {
  if (M <= 0 || E <= 0 || E % 128 || E > 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vcap_ln_backward_kernel<false>, dim3((M + 3) / 4), dim3(256), 0, s, x, dy, gamma, eps, M, E, g,
                     (float*)nullptr);
  return hipGetLastError();
}

hipError_t vcap_ln_backward_stats_dispatch(const float* x, const float* dy, const float* gamma, float eps, int M,
                                           int E, float* g, float* stats, hipStream_t s) {
  if (M <= 0 || E <= 0 || E % 128 || E > 1024 || !stats) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vcap_ln_backward_kernel<true>, dim3((M + 3) / 4), dim3(256), 0, s, x, dy, gamma, eps, M, E, g,
                     stats);
  return hipGetLastError();
}

hipError_t vcap_gelu_backward_dispatch(int dt, const float* u, const float* dact, long n, void* du, hipStream_t s) {
  if (n <= 0) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if (dt == VCAP_DT_BF16)
    hipLaunchKernelGGL(vcap_gelu_backward_kernel<bf16_t>, grid, block, 0, s, u, dact, n, (bf16_t*)du);
  else if (dt == VCAP_DT_F32)
    hipLaunchKernelGGL(vcap_gelu_backward_kernel<float>, grid, block, 0, s, u, dact, n, (float*)du);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t vcap_grad_to_bf16_dispatch(const float* x, long n, void* y, hipStream_t s) {
  if (n <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vcap_grad_to_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, (bf16_t*)y);
  return hipGetLastError();
}

hipError_t vcap_attn_backward_dispatch(int dt, const float* qkv, const float* dO, const uint8_t* kmask, int B, int S,
                                       int H, float* P, float* dS, void* dqkv, hipStream_t s) {
  if (B <= 0 || S <= 0 || S > 512 || H <= 0) return hipErrorInvalidValue;
  const dim3 grid((S + 3) / 4, B * H), block(256);
  hipLaunchKernelGGL(vcap_attn_bwd_rows_kernel, grid, block, 0, s, qkv, dO, kmask, S, H, P, dS);
  if (hipError_t e = hipGetLastError()) return e;
  if (dt == VCAP_DT_BF16)
    hipLaunchKernelGGL(vcap_attn_bwd_sums_kernel<bf16_t>, grid, block, 0, s, qkv, dO, (const float*)P,
                       (const float*)dS, S, H, (bf16_t*)dqkv);
  else if (dt == VCAP_DT_F32)
    hipLaunchKernelGGL(vcap_attn_bwd_sums_kernel<float>, grid, block, 0, s, qkv, dO, (const float*)P, (const float*)dS,
                       S, H, (float*)dqkv);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t vcap_grad_finish_dispatch(const float* g, const uint8_t* kmask, int B, int S, int E, float* out,
                                     hipStream_t s) {
  const long n = (long)B * S * E;
  if (n <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vcap_grad_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, kmask, S, E, n,
                     out);
  return hipGetLastError();
}
