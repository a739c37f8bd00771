// Kernels of vcap_text_encode_backward (schedule: runtime_text_grad.hip): the gradient of any scalar of the
// text tower's unit-norm output rows with respect to every text-tower parameter - the embedding table,
// every nn.TransformerEncoderLayer weight, bias and LayerNorm affine, and txt_proj.
//
//   vcap_text_tail_bwd_kernel     per caption: pooled, y = proj(pooled) + b and ||y|| recomputed exactly as
//                                 vcap_text_pool_kernel computes them, dy = (g - out (out . g)) / ||y|| (g / eps
//                                 below the eps), dpooled = dy . proj_w, dhidden = mask / max(count, 1) dpooled
//   vcap_text_proj_grad_kernel    dproj_w[p][e] = sum over captions in order of dy[b][p] pooled[b][e]; dproj_b
//   vcap_text_ln_bwd_kernel       the LayerNorm input gradient of dy = a (+ b) at the rows x; one wave per row;
//                                 leaves the summed dy in a and the row's (mean, rstd) for the column sums
//   vcap_text_colsum_kernel       bias gradients: out[c] = sum_m src[m][c] (rows f32, or the decoder dtype for the
//                                 GPT-2 tail's bias gradients: vcap_colsum_dispatch); with the rows x and their stats:
//                                 dgamma[c] = sum_m dy[m][c] xhat[m][c] and dbeta[c] = sum_m dy[m][c]
//   vcap_text_transpose_kernel    src [M][N] (f32 or T) -> dst [N][Mpad] in T through a 32 x 64 LDS tile, columns
//                                 m >= M written as +0: the K-contiguous operands dY^T and X^T of
//                                 dW = dY^T . X on vcap_grad_gemm_kernel (K = Mpad)
//   vcap_text_relu_bwd_kernel     du = dact where the stored ReLU output is > 0 (or dact is NaN), else +0
//   vcap_text_attn_bwd_rows_kernel / _sums_kernel   bidirectional attention backward, f32 throughout: one wave
//                                 per (caption, head, query) writes the P and dS rows, then one wave per
//                                 (caption, head, position) sums dq, dk, dv in index order
//   vcap_text_emb_slots_kernel    the distinct non-pad ids of the call in ascending order and each position's slot
//   vcap_text_emb_rows_kernel     row i = the sum of dx0 over the positions holding emb_ids[i], in position order
//
// Every reduction over the M = B L rows has one order, a function of M alone: wave w of a column's workgroup
// adds rows w, w + 4, ... in order and the four partial sums are added in wave order (column sums); K tiles
// of 128 bytes in order inside constant 128-column slabs that vcap_grad_slab_sum_kernel adds in slab order
// (weight gradients).  Nothing is accumulated atomically.
//
// Exact zeros: accumulators start at +0 and only add, and the element-wise kernels end in "+ 0.f", so rows
// whose incoming gradient is all +0 leave every kernel as +0 and add +0 to every sum over rows.
#include "vcap_common.h"
#include "vcap_kernels.h"

namespace {

VCAP_DEV float lane_bcast(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// One workgroup of 16 waves per caption; pooled, y and the norm as in vcap_text_pool_kernel (same
// expressions, same orders), so out == y / max(||y||, 1e-12) to the bit.
__global__ __launch_bounds__(1024) void vcap_text_tail_bwd_kernel(
    const float* __restrict__ x, const int* __restrict__ ids, int pad_id, int L, int E, const float* __restrict__ pw,
    const float* __restrict__ pb, int P, const float* __restrict__ out, const float* __restrict__ gout,
    float* __restrict__ dy, float* __restrict__ pooled_out, float* __restrict__ g) {
  __shared__ __attribute__((aligned(16))) float pooled[1024];
  __shared__ float yv[1024];
  __shared__ float dyv[1024];
  __shared__ float keep[64];
  __shared__ float s_raw, s_dot, s_cnt;
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
    const float pv = acc / fmaxf(cnt, 1.f);
    pooled[tid] = pv;
    pooled_out[(long)b * E + tid] = pv;
    if (tid == 0) s_cnt = fmaxf(cnt, 1.f);
  }
  __syncthreads();
  const int nc = E / 128, per_wave = P / 16;
  for (int k = 0; k < per_wave; ++k) {
    const int p = wave * per_wave + k;
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (c < nc) {
        const f32x2 w = *reinterpret_cast<const f32x2*>(pw + (long)p * E + c * 128 + lane * 2);
        const f32x2 pv = *reinterpret_cast<const f32x2*>(pooled + c * 128 + lane * 2);
        acc = fmaf(w.x, pv.x, fmaf(w.y, pv.y, acc));
      }
    acc = wave_sum(acc);
    if (lane == 0) yv[p] = acc + pb[p];
  }
  __syncthreads();
  if (wave == 0) {
    float ss = 0.f, dt = 0.f;
    for (int p = lane; p < P; p += 64) {
      ss = fmaf(yv[p], yv[p], ss);
      dt = fmaf(out[(long)b * P + p], gout[(long)b * P + p], dt);
    }
    ss = wave_sum(ss);
    dt = wave_sum(dt);
    if (lane == 0) {
      s_raw = sqrtf(ss);
      s_dot = dt;
    }
  }
  __syncthreads();
  if (tid < P) {
    const float gv = gout[(long)b * P + tid], ov = out[(long)b * P + tid];
    // a NaN norm (an id outside the vocabulary) takes the first form and stays NaN
    const float v = !(s_raw <= 1e-12f) ? (gv - ov * s_dot) / s_raw : gv / 1e-12f;
    dyv[tid] = v;
    dy[(long)b * P + tid] = v;
  }
  __syncthreads();
  if (tid < E) {
    float acc = 0.f;
    for (int p = 0; p < P; ++p) acc = fmaf(dyv[p], pw[(long)p * E + tid], acc);
    const float dp = acc / s_cnt;
    for (int l = 0; l < L; ++l) g[((long)b * L + l) * E + tid] = keep[l] != 0.f ? dp + 0.f : 0.f;
  }
}

// grid P, 256 threads: row p of dproj_w, captions in order; thread 0 also sums dproj_b[p]
__global__ __launch_bounds__(256) void vcap_text_proj_grad_kernel(const float* __restrict__ dy,
                                                                  const float* __restrict__ pooled, int B, int E,
                                                                  int P, float* __restrict__ dw,
                                                                  float* __restrict__ db) {
  const int p = blockIdx.x;
  for (int e = threadIdx.x; e < E; e += 256) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc = fmaf(dy[(long)b * P + p], pooled[(long)b * E + e], acc);
    dw[(long)p * E + e] = acc;
  }
  if (threadIdx.x == 0) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc += dy[(long)b * P + p];
    db[p] = acc;
  }
}

// ------------------------------------------------------------------------------------------------
// dx[m] = rstd (dyh - mean(dyh) - xh mean(dyh xh)), dyh = dy gamma, xh = (x - mean) rstd, dy = a (+ b).
// One row per wave, lane l holds columns 128 k + 2 l + {0, 1}, k < E / 128 <= 8.  a <- dy; stats[m] = (mean, rstd).
__global__ __launch_bounds__(256) void vcap_text_ln_bwd_kernel(const float* __restrict__ x, float* __restrict__ a,
                                                               const float* __restrict__ b,
                                                               const float* __restrict__ gamma, float eps, int M,
                                                               int E, float* __restrict__ dx,
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
      f32x2 d = *reinterpret_cast<const f32x2*>(a + o);
      if (b) {
        d = d + *reinterpret_cast<const f32x2*>(b + o);
        *reinterpret_cast<f32x2*>(a + o) = d;
      }
      dv[k] = d * *reinterpret_cast<const f32x2*>(gamma + k * 128 + 2 * lane);
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
  if (lane == 0) *reinterpret_cast<f32x2*>(stats + 2L * row) = (f32x2){mean, rstd};
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
      f32x2 r;
      r.x = rstd * (dv[k].x - m1 - xv[k].x * m2) + 0.f;
      r.y = rstd * (dv[k].y - m1 - xv[k].y * m2) + 0.f;
      *reinterpret_cast<f32x2*>(dx + o) = r;
    }
}

// grid N / 64, 256 threads: lane -> column, wave w -> rows w, w + 4, ... in order; the four partial sums are
// added in wave order.  With x and stats: out = sum dy xhat (dgamma) and out2 = sum dy (dbeta); without: out =
// sum src (a bias gradient).  S: the rows' dtype (f32 here; the GPT-2 tail's bias gradients sum rows of the
// decoder dtype, vcap_colsum_dispatch); the sums are f32.
template <typename S>
__global__ __launch_bounds__(256) void vcap_text_colsum_kernel(const S* __restrict__ src,
                                                               const float* __restrict__ x,
                                                               const float* __restrict__ stats, int M, int N,
                                                               float* __restrict__ out, float* __restrict__ out2) {
  __shared__ float part[2][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  float s = 0.f, sx = 0.f;
  for (int m = wave; m < M; m += 4) {
    const float d = Num<S>::to_f(src[(long)m * N + c]);
    s += d;
    if (x) {
      const f32x2 st = *reinterpret_cast<const f32x2*>(stats + 2L * m);
      sx = fmaf(d, (x[(long)m * N + c] - st.x) * st.y, sx);
    }
  }
  part[0][wave][lane] = s;
  part[1][wave][lane] = sx;
  __syncthreads();
  if (wave == 0) {
    const float t = ((part[0][0][lane] + part[0][1][lane]) + part[0][2][lane]) + part[0][3][lane];
    const float tx = ((part[1][0][lane] + part[1][1][lane]) + part[1][2][lane]) + part[1][3][lane];
    if (x) {
      out[c] = tx;
      out2[c] = t;
    } else {
      out[c] = t;
    }
  }
}

// grid (N / 64, Mpad / 32), 256 threads.  N % 64 == 0, Mpad % 32 == 0, Mpad >= M.
template <typename S, typename T>
__global__ __launch_bounds__(256) void vcap_text_transpose_kernel(const S* __restrict__ src, int M, int N, int Mpad,
                                                                  T* __restrict__ dst) {
  __shared__ float tile[32][65];
  const int t = threadIdx.x;
  const int n0 = blockIdx.x * 64, m0 = blockIdx.y * 32;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int ml = (t >> 6) + 4 * i, nl = t & 63;
    const int m = m0 + ml;
    tile[ml][nl] = m < M ? Num<S>::to_f(src[(long)m * N + n0 + nl]) : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int nl = (t >> 5) + 8 * i, ml = t & 31;
    dst[(long)(n0 + nl) * Mpad + m0 + ml] = Num<T>::from_f(tile[ml][nl]);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void vcap_text_relu_bwd_kernel(const T* __restrict__ act, long n,
                                                                 float* __restrict__ d) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  // a NaN gradient (an id outside the vocabulary: the forward's fmaxf stores that caption's activations as 0)
  // passes the mask, so the bias gradient of linear1 is NaN like every other gradient of such a call
  if (i < n) {
    const float g = d[i];
    d[i] = (Num<T>::to_f(act[i]) > 0.f || g != g) ? g + 0.f : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------
// grid (ceil(L / 4), B * H): wave -> query i, lane -> key j (and head dimension d for the query's own rows).
// qkv [B*L][3E] T as the forward stored it, dO [B*L][E] f32; P, dS [B*H][L][L] f32.  The scores and P are
// vcap_text_attention_kernel's: sum over d in order of (q[i][d] / 8) k[j][d], exp(s - max) / sum.
// dS = P (dP - sum_j P dP) / 8, dP[j] = sum over d in order of dO[i][d] v[j][d].
template <typename T>
__global__ __launch_bounds__(256) void vcap_text_attn_bwd_rows_kernel(const T* __restrict__ qkv,
                                                                      const float* __restrict__ dO, int L, int H,
                                                                      float* __restrict__ P, float* __restrict__ dS) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= L) return;
  const int b = blockIdx.y / H, h = blockIdx.y - b * H;
  const int E = H * 64;
  const long ld = 3L * E;
  const T* base = qkv + (long)b * L * ld + h * 64;
  const float qv = Num<T>::to_f(base[(long)i * ld + lane]) * 0.125f;
  const float ov = dO[((long)b * L + i) * E + h * 64 + lane];
  const T* kr = base + (long)min(lane, L - 1) * ld + E;  // clamped: lanes >= L are discarded below
  const T* vr = kr + E;
  float s = 0.f, dp = 0.f;
#pragma unroll
  for (int d = 0; d < 64; ++d) {
    s = fmaf(lane_bcast(qv, d), Num<T>::to_f(kr[d]), s);
    dp = fmaf(lane_bcast(ov, d), Num<T>::to_f(vr[d]), dp);
  }
  const bool live = lane < L;
  s = live ? s : -INFINITY;
  dp = live ? dp : 0.f;
  const float mx = wave_max(s);
  float p = expf(s - mx);
  p = p / wave_sum(p);
  const float dl = wave_sum(p * dp);
  if (live) {
    const long o = ((long)blockIdx.y * L + i) * L + lane;
    P[o] = p;
    dS[o] = p * (dp - dl) * 0.125f + 0.f;
  }
}

// grid (ceil(L / 4), B * H): wave -> position r, lane -> head dimension d.  dqkv [B*L][3E] f32.
// dq_r = sum_j dS[r][j] k_j, dk_r = sum_i dS[i][r] q_i, dv_r = sum_i P[i][r] dO_i, each in index order.
template <typename T>
__global__ __launch_bounds__(256) void vcap_text_attn_bwd_sums_kernel(const T* __restrict__ qkv,
                                                                      const float* __restrict__ dO,
                                                                      const float* __restrict__ P,
                                                                      const float* __restrict__ dS, int L, int H,
                                                                      float* __restrict__ dqkv) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= L) return;
  const int b = blockIdx.y / H, h = blockIdx.y - b * H;
  const int E = H * 64;
  const long ld = 3L * E;
  const T* q0 = qkv + (long)b * L * ld + h * 64 + lane;
  const float* o0 = dO + (long)b * L * E + h * 64 + lane;
  const float* Pb = P + (long)blockIdx.y * L * L;
  const float* Sb = dS + (long)blockIdx.y * L * L;
  float dq = 0.f, dk = 0.f, dv = 0.f;
  for (int j = 0; j < L; ++j) {
    dq = fmaf(Sb[(long)r * L + j], Num<T>::to_f(q0[(long)j * ld + E]), dq);
    dk = fmaf(Sb[(long)j * L + r], Num<T>::to_f(q0[(long)j * ld]), dk);
    dv = fmaf(Pb[(long)j * L + r], o0[(long)j * E], dv);
  }
  float* out = dqkv + ((long)b * L + r) * ld + h * 64 + lane;
  out[0] = dq;
  out[E] = dk;
  out[2 * E] = dv;
}

// ------------------------------------------------------------------------------------------------
// One workgroup of 512 threads, M <= 512.  slot[m] = the rank of ids[m] among the call's distinct non-pad
// ids inside the vocabulary, -1 for a pad or an id outside it (which is never used as an index);
// emb_ids[rank] = the id, -1 from count up; *count = the number of distinct ids.
__global__ __launch_bounds__(512) void vcap_text_emb_slots_kernel(const int* __restrict__ ids, int M, int pad_id,
                                                                  int vocab, int* __restrict__ slot,
                                                                  int* __restrict__ emb_ids,
                                                                  int* __restrict__ count) {
  __shared__ int sid[512];
  __shared__ int sfirst[512];
  const int m = threadIdx.x;
  int id = -1;
  if (m < M) {
    const int v = ids[m];
    if (v != pad_id && (unsigned)v < (unsigned)vocab) id = v;
  }
  sid[m] = id;
  __syncthreads();
  int first = id >= 0;
  for (int j = 0; j < m && first; ++j) first = sid[j] != id;
  sfirst[m] = first;
  const int total = __syncthreads_count(first);
  int rank = 0;
  for (int j = 0; j < M; ++j) rank += (sfirst[j] && sid[j] < id) ? 1 : 0;
  if (m < M) {
    slot[m] = id >= 0 ? rank : -1;
    if (m >= total) emb_ids[m] = -1;
  }
  if (first) emb_ids[rank] = id;
  if (m == 0) *count = total;
}

// grid M, 256 threads: row i = sum over the positions m in order with slot[m] == i of (a[m] + b[m]), from +0
__global__ __launch_bounds__(256) void vcap_text_emb_rows_kernel(const float* __restrict__ a,
                                                                 const float* __restrict__ b,
                                                                 const int* __restrict__ slot, int M, int E,
                                                                 float* __restrict__ rows) {
  __shared__ int ss[512];
  const int i = blockIdx.x;
  for (int m = threadIdx.x; m < M; m += 256) ss[m] = slot[m];
  __syncthreads();
  for (int e = threadIdx.x; e < E; e += 256) {
    float acc = 0.f;
    for (int m = 0; m < M; ++m)
      if (ss[m] == i) {
        float v = a[(long)m * E + e];
        if (b) v += b[(long)m * E + e];
        acc += v;
      }
    rows[(long)i * E + e] = acc;
  }
}

// ---- dispatchers ------------------------------------------------------------------------------------
hipError_t vcap_text_tail_bwd_dispatch(const float* x, const int* ids, int pad_id, int B, int L, int E,
                                       const float* pw, const float* pb, int P, const float* out, const float* gout,
                                       float* dy, float* pooled, float* g, float* dproj_w, float* dproj_b,
                                       hipStream_t s) {
  if (B <= 0 || L < 1 || L > 64 || E <= 0 || E % 128 || E > 1024 || P < 64 || P % 64 || P > 1024)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(vcap_text_tail_bwd_kernel, dim3(B), dim3(1024), 0, s, x, ids, pad_id, L, E, pw, pb, P, out, gout,
                     dy, pooled, g);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(vcap_text_proj_grad_kernel, dim3(P), dim3(256), 0, s, (const float*)dy, (const float*)pooled, B,
                     E, P, dproj_w, dproj_b);
  return hipGetLastError();
}

hipError_t vcap_text_ln_bwd_dispatch(const float* x, float* a, const float* b, const float* gamma, float eps, int M,
                                     int E, float* dx, float* stats, float* dgamma, float* dbeta, hipStream_t s) {
  if (M <= 0 || E <= 0 || E % 128 || E > 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vcap_text_ln_bwd_kernel, dim3((M + 3) / 4), dim3(256), 0, s, x, a, b, gamma, eps, M, E, dx, stats);
  if (hipError_t e = hipGetLastError()) return e;
  return vcap_ln_colsum_dispatch(a, x, stats, M, E, dgamma, dbeta, s);
}

hipError_t vcap_ln_colsum_dispatch(const float* dy, const float* x, const float* stats, int M, int E, float* dgamma,
                                   float* dbeta, hipStream_t s) {
  if (M <= 0 || E <= 0 || E % 64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vcap_text_colsum_kernel<float>, dim3(E / 64), dim3(256), 0, s, dy, x, stats, M, E, dgamma, dbeta);
  return hipGetLastError();
}

hipError_t vcap_text_colsum_dispatch(const float* src, int M, int N, float* out, hipStream_t s) {
  return vcap_colsum_dispatch(VCAP_DT_F32, src, M, N, out, s);
}

hipError_t vcap_colsum_dispatch(int dt, const void* src, int M, int N, float* out, hipStream_t s) {
  if (M <= 0 || N <= 0 || N % 64) return hipErrorInvalidValue;
  if (dt == VCAP_DT_F32)
    hipLaunchKernelGGL(vcap_text_colsum_kernel<float>, dim3(N / 64), dim3(256), 0, s, (const float*)src,
                       (const float*)nullptr, (const float*)nullptr, M, N, out, (float*)nullptr);
  else if (dt == VCAP_DT_BF16)
    hipLaunchKernelGGL(vcap_text_colsum_kernel<bf16_t>, dim3(N / 64), dim3(256), 0, s, (const bf16_t*)src,
                       (const float*)nullptr, (const float*)nullptr, M, N, out, (float*)nullptr);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t vcap_text_transpose_dispatch(int dt, int src_f32, const void* src, int M, int N, int Mpad, void* dst,
                                        hipStream_t s) {
  if (M <= 0 || N <= 0 || N % 64 || Mpad < M || Mpad % 32) return hipErrorInvalidValue;
  const dim3 grid(N / 64, Mpad / 32), block(256);
  if (dt == VCAP_DT_F32)
    hipLaunchKernelGGL((vcap_text_transpose_kernel<float, float>), grid, block, 0, s, (const float*)src, M, N, Mpad,
                       (float*)dst);
  else if (dt == VCAP_DT_BF16 && src_f32)
    hipLaunchKernelGGL((vcap_text_transpose_kernel<float, bf16_t>), grid, block, 0, s, (const float*)src, M, N, Mpad,
                       (bf16_t*)dst);
  else if (dt == VCAP_DT_BF16)
    hipLaunchKernelGGL((vcap_text_transpose_kernel<bf16_t, bf16_t>), grid, block, 0, s, (const bf16_t*)src, M, N,
                       Mpad, (bf16_t*)dst);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t vcap_text_relu_bwd_dispatch(int dt, const void* act, long n, float* d, hipStream_t s) {
  if (n <= 0) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if (dt == VCAP_DT_BF16)
    hipLaunchKernelGGL(vcap_text_relu_bwd_kernel<bf16_t>, grid, block, 0, s, (const bf16_t*)act, n, d);
  else if (dt == VCAP_DT_F32)
    hipLaunchKernelGGL(vcap_text_relu_bwd_kernel<float>, grid, block, 0, s, (const float*)act, n, d);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t vcap_text_attn_bwd_dispatch(int dt, const void* qkv, const float* dO, int B, int L, int H, float* P,
                                       float* dS, float* dqkv, hipStream_t s) {
  if (B <= 0 || H <= 0 || L < 1 || L > 64) return hipErrorInvalidValue;
  const dim3 grid((L + 3) / 4, B * H), block(256);
  if (dt == VCAP_DT_BF16) {
    hipLaunchKernelGGL(vcap_text_attn_bwd_rows_kernel<bf16_t>, grid, block, 0, s, (const bf16_t*)qkv, dO, L, H, P, dS);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(vcap_text_attn_bwd_sums_kernel<bf16_t>, grid, block, 0, s, (const bf16_t*)qkv, dO,
                       (const float*)P, (const float*)dS, L, H, dqkv);
  } else if (dt == VCAP_DT_F32) {
    hipLaunchKernelGGL(vcap_text_attn_bwd_rows_kernel<float>, grid, block, 0, s, (const float*)qkv, dO, L, H, P, dS);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(vcap_text_attn_bwd_sums_kernel<float>, grid, block, 0, s, (const float*)qkv, dO,
                       (const float*)P, (const float*)dS, L, H, dqkv);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t vcap_text_emb_grad_dispatch(const int* ids, int M, int pad_id, int vocab, const float* a, const float* b,
                                       int E, int* slot, int* emb_ids, int* count, float* rows, hipStream_t s) {
  if (M <= 0 || M > 512 || E <= 0 || vocab <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vcap_text_emb_slots_kernel, dim3(1), dim3(512), 0, s, ids, M, pad_id, vocab, slot, emb_ids, count);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(vcap_text_emb_rows_kernel, dim3(M), dim3(256), 0, s, a, b, (const int*)slot, M, E, rows);
  return hipGetLastError();
}
