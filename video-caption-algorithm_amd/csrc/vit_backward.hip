// Kernels of vcap_vit_encode_backward and vcap_vit_attention_backward (schedule: runtime_vit_grad.hip): the
// gradient of any scalar of the encoder output with respect to the ViT's parameters.
//
//   vcap_vit_attn_bwd_probs_kernel<T>   per (frame, head, 16-query tile), one wave, on the MFMA: S = Q K^T, the
//                                       forward's softmax expression exp2((s - max) * log2(e) / 8) / sum, dP = dO V^T,
//                                       delta = rowsum(exp . dP) / sum, dS = P (dP - delta) / 8.  Both products
//                                       contract the head dimension, so every fragment is one 16-byte load of a
//                                       row of q | k | v or dO as it lies in HBM.  Three sweeps over the key tiles
//                                       (max; sum and delta; P and dS) recompute S and dP instead of holding
//                                       <= 18 tiles of each in registers: no register array indexed by a runtime
//                                       tile count, no scratch.  Writes P, dS ([query][key]) and dS^T ([key][query])
//                                       in the operand dtype to the workspace.
//   vcap_vit_xty_kernel<T>              C[k][n] = sum_m X[m][k] Y[m][n] over row-major X and Y, both operands
//                                       read column-wise from LDS (ds_read_b64_tr_b16 for bf16, ds_read_b32 for
//                                       f32) as vcap_gpt2_dw_kernel reads them, a 64 x 64 output tile per
//                                       workgroup, at every row count.  grid.z batches: the (frame, head) pairs
//                                       of dQ = (dS^T)^T K, dK = dS^T Q, dV = P^T dO, or the constant 256-row slabs
//                                       of a weight gradient dW = dY^T X, which vcap_grad_slab_sum_kernel adds in
//                                       slab order.
//   vcap_vit_head_bwd_kernel            per video: pooled = mean_t of the final-norm CLS rows, dpooled =
//                                       grad_out . proj_w, d(norm row) = dpooled / T
//   vcap_vit_proj_grad_kernel           encoder.proj dW / db, videos in order
//   vcap_vit_pos_grad_kernel            dpos[n] = sum over frames in order of g[frame][n]; dcls = dpos[0]
//   vcap_vit_rows_copy_kernel           strided f32 row copies: the CLS rows in and out of their compact form,
//                                       the patch rows of the embedding gradient
//
// f32 operands: the same kernels on the f32-input MFMA (16x16x4), P / dS kept in f32; nothing is rounded.
// bf16 rounding points (RNE), everything else f32: q | k | v as the forward stored them; dO, P, dS and every
// row gradient that enters a product (dY of each Linear) once, when it becomes an MFMA operand.  The residual
// gradient, the softmax, delta, the LayerNorm and GELU backward, bias / gamma / beta sums and all
// accumulators are f32.
//
// Orders: a sum over keys or queries inside one (frame, head) is one wave's ascending 32-row tiles; a sum
// over the M rows of a weight gradient is ascending 32-row tiles inside 256-row slabs, slabs added in
// order.  None depends on the grid, a CU mask or the call's history; nothing is accumulated atomically.
//
// Exact zeros: accumulators start at +0 and only add; a key at or past the token count has P = dS = +0;
// dO = +0 rows give dP = delta = +0 and dS = P (0 - 0) / 8 + 0 = +0.
#include "vcap_common.h"
#include "vcap_kernels.h"

namespace {

// ds_read_b64_tr_b16 column fragments of a row-major bf16 LDS image (gpt2_weight_grad.hip's address function)
VCAP_DEV u32x2 tr_read16(const char* p) {
  typedef __attribute__((ext_vector_type(4))) short s16x4;
  const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
  return __builtin_bit_cast(u32x2, v);
}
// rows 8 fg .. 8 fg + 7 of column c0 + fr
VCAP_DEV u32x4 col_frag16(const char* img, int stride, int c0, int fr, int fg) {
  const char* p = img + (8 * fg + (fr >> 2)) * stride + (c0 + 4 * (fr & 3)) * 2;
  const u32x2 lo = tr_read16(p), hi = tr_read16(p + 4 * stride);
  return (u32x4){lo.x, lo.y, hi.x, hi.y};
}

constexpr int XT = 64, XRM = 32;   // xty: output tile edge, rows per reduction step
template <typename T>
struct XtyTile {
  static constexpr int PAD = sizeof(T) == 2 ? 16 : 64;
  static constexpr int RS = XT * (int)sizeof(T) + PAD;    // row stride of an LDS image, bytes
  static constexpr int IMG = XRM * RS;
  static constexpr int EPC = 16 / (int)sizeof(T);         // elements per 16-byte chunk
  static constexpr int CPR = XT / EPC;                    // chunks per image row
  static constexpr int CL = XRM * CPR / 256;              // chunks per thread
};

// chunk idx of a [XRM][XT] tile at (m0, c0): zeros at and past `rows` rows or `cols` columns
template <typename T>
VCAP_DEV u32x4 xty_chunk(const T* __restrict__ P, long ld, int c0, int cols, int m0, int rows, int idx) {
  const int r = idx / XtyTile<T>::CPR, c = c0 + (idx % XtyTile<T>::CPR) * XtyTile<T>::EPC;
  if (m0 + r >= rows || c >= cols) return (u32x4){0u, 0u, 0u, 0u};
  return *reinterpret_cast<const u32x4*>(P + (long)(m0 + r) * ld + c);
}

VCAP_DEV void xty_mma(const char* xs, const char* ys, int wk, int wn, int fr, int fg, f32x4 (&acc)[2][2], bf16_t*) {
  typedef XtyTile<bf16_t> D;
  u32x4 xf[2], yf[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) xf[i] = col_frag16(xs, D::RS, wk * 32 + i * 16, fr, fg);
#pragma unroll
  for (int j = 0; j < 2; ++j) yf[j] = col_frag16(ys, D::RS, wn * 32 + j * 16, fr, fg);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = mfma_frag(yf[j], xf[i], acc[i][j], (bf16_t*)nullptr);
}

VCAP_DEV void xty_mma(const char* xs, const char* ys, int wk, int wn, int fr, int fg, f32x4 (&acc)[2][2], float*) {
  typedef XtyTile<float> D;
#pragma unroll
  for (int s = 0; s < XRM / 4; ++s) {
    const int r = 4 * s + fg;
    float xv[2], yv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) xv[i] = *reinterpret_cast<const float*>(xs + r * D::RS + (wk * 32 + i * 16 + fr) * 4);
#pragma unroll
    for (int j = 0; j < 2; ++j) yv[j] = *reinterpret_cast<const float*>(ys + r * D::RS + (wn * 32 + j * 16 + fr) * 4);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[j], xv[i], acc[i][j], 0, 0, 0);
  }
}

// the score and dP tiles of key tile kt for the wave's 16 queries: lane (fr, fg) holds query 4 fg + e, key
// 16 kt + fr.  Rows at and past N are the clamped row N - 1 (finite; masked or unused by the caller).
template <typename T, int KS, bool WITH_DP>
VCAP_DEV void attn_tiles(const T* __restrict__ kb, const T* __restrict__ vb, long ld, int key, const u32x4 (&qf)[KS],
                         const u32x4 (&of)[KS], f32x4& s, f32x4& dp) {
  constexpr int KE = Frag<T>::kElems;
  const int fg = (threadIdx.x & 63) >> 4;
  s = (f32x4){0.f, 0.f, 0.f, 0.f};
  dp = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    const u32x4 kf = *reinterpret_cast<const u32x4*>(kb + (long)key * ld + k * 4 * KE + fg * KE);
    s = mfma_frag(qf[k], kf, s, (T*)nullptr);
    if constexpr (WITH_DP) {
      const u32x4 vf = *reinterpret_cast<const u32x4*>(vb + (long)key * ld + k * 4 * KE + fg * KE);
      dp = mfma_frag(of[k], vf, dp, (T*)nullptr);
    }
  }
}

}  // namespace

// grid (ceil(N / 64), frames * H), 256 threads: wave w of block x owns queries 16 (4 x + w) .. + 15.
// qkv [frames * N][3 * 64 H] T, dO [frames * N][64 H] T; P, dS, dST: [frames * H][ldp][ldp] T, ldp = N rounded
// up to 64.
template <typename T>
__global__ __launch_bounds__(256) void vcap_vit_attn_bwd_probs_kernel(const T* __restrict__ qkv,
                                                                      const T* __restrict__ dO, int N, int H, int ldp,
                                                                      T* __restrict__ P, T* __restrict__ dS,
                                                                      T* __restrict__ dST) {
  constexpr int KE = Frag<T>::kElems;    // elements per 16-byte fragment
  constexpr int KS = 64 / (4 * KE);      // MFMA K steps over the head dimension
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fg = lane >> 4;
  const int q0 = (blockIdx.x * 4 + wave) * 16;
  if (q0 >= N) return;   // wave-uniform; the kernel has no barrier
  const int bh = blockIdx.y, f = bh / H, h = bh - f * H;
  const int D = 64 * H;
  const long ld = 3L * D;
  const T* qb = qkv + (long)f * N * ld + h * 64;
  const T* kb = qb + D;
  const T* vb = kb + D;
  const T* ob = dO + (long)f * N * D + h * 64;
  const int qrow = min(q0 + fr, N - 1);
  u32x4 qf[KS], of[KS];
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    qf[k] = *reinterpret_cast<const u32x4*>(qb + (long)qrow * ld + k * 4 * KE + fg * KE);
    of[k] = *reinterpret_cast<const u32x4*>(ob + (long)qrow * D + k * 4 * KE + fg * KE);
  }
  const float c2 = 0.125f * 1.4426950408889634f;   // 64^-0.5 * log2(e), as the forward kernels
  const int nkt = (N + 15) >> 4;
  f32x4 s, dp;
  float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int kt = 0; kt < nkt; ++kt) {
    const int key = kt * 16 + fr;
    attn_tiles<T, KS, false>(kb, vb, ld, min(key, N - 1), qf, of, s, dp);
#pragma unroll
    for (int e = 0; e < 4; ++e) mx[e] = fmaxf(mx[e], key < N ? s[e] : -INFINITY);
  }
  float mxc[4], sum[4] = {0.f, 0.f, 0.f, 0.f}, du[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e) mxc[e] = row16_max(mx[e]) * c2;
  for (int kt = 0; kt < nkt; ++kt) {
    const int key = kt * 16 + fr;
    attn_tiles<T, KS, true>(kb, vb, ld, min(key, N - 1), qf, of, s, dp);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float p = key < N ? __builtin_amdgcn_exp2f(fmaf(s[e], c2, -mxc[e])) : 0.f;
      sum[e] += p;
      du[e] = fmaf(p, dp[e], du[e]);
    }
  }
  float inv[4], dl[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    inv[e] = 1.0f / row16_sum(sum[e]);
    dl[e] = row16_sum(du[e]) * inv[e];
  }
  T* Pb = P + (long)bh * ldp * ldp;
  T* Sb = dS + (long)bh * ldp * ldp;
  T* Tb = dST + (long)bh * ldp * ldp;
  for (int kt = 0; kt < nkt; ++kt) {
    const int key = kt * 16 + fr;
    attn_tiles<T, KS, true>(kb, vb, ld, min(key, N - 1), qf, of, s, dp);
    float pv[4], dv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      pv[e] = key < N ? __builtin_amdgcn_exp2f(fmaf(s[e], c2, -mxc[e])) * inv[e] : 0.f;
      dv[e] = pv[e] * (dp[e] - dl[e]) * 0.125f + 0.f;
      const long o = (long)(q0 + 4 * fg + e) * ldp + key;   // rows < 16 ceil(N / 16) <= ldp, key < ldp
      Pb[o] = Num<T>::from_f(pv[e]);
      Sb[o] = Num<T>::from_f(dv[e]);
    }
    T* t = Tb + (long)key * ldp + q0 + 4 * fg;
    if constexpr (sizeof(T) == 2)
      *reinterpret_cast<u32x2*>(t) = (u32x2){pack_bf2(dv[0], dv[1]), pack_bf2(dv[2], dv[3])};
    else
      *reinterpret_cast<f32x4*>(t) = (f32x4){dv[0], dv[1], dv[2], dv[3]};
  }
}

// grid (ceil(K / 64), ceil(N / 64), Z), 256 threads (2 x 2 waves of 32 x 32).  Batch z = (z1, z2) = (z / Z2,
// z % Z2) reads rows [0, min(slab_rows, rows_total - z1 * slab_step)) of X + z1 xs1 + z2 xs2 and Y + ..., and
// writes C + z1 cs1 + z2 cs2.
template <typename T>
__global__ __launch_bounds__(256) void vcap_vit_xty_kernel(XtyArgs a) {
  typedef XtyTile<T> D;
  __shared__ __attribute__((aligned(16))) char smem[2 * D::IMG];
  char* xs = smem;
  char* ys = smem + D::IMG;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wk = wave >> 1, wn = wave & 1, fr = lane & 15, fg = lane >> 4;
  const int k0 = blockIdx.x * XT, n0 = blockIdx.y * XT;
  const int z1 = blockIdx.z / a.Z2, z2 = blockIdx.z - z1 * a.Z2;
  const T* X = (const T*)a.X + z1 * a.xs1 + z2 * a.xs2;
  const T* Y = (const T*)a.Y + z1 * a.ys1 + z2 * a.ys2;
  float* C = a.C + z1 * a.cs1 + z2 * a.cs2;
  const int rows = min(a.slab_rows, a.rows_total - z1 * a.slab_step);
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  u32x4 xr[D::CL], yr[D::CL];
#pragma unroll
  for (int i = 0; i < D::CL; ++i) {
    xr[i] = xty_chunk<T>(X, a.ldx, k0, a.Kmem, 0, rows, tid + 256 * i);
    yr[i] = xty_chunk<T>(Y, a.ldy, n0, a.N, 0, rows, tid + 256 * i);
  }
  const int nmt = (rows + XRM - 1) / XRM;
  for (int mt = 0; mt < nmt; ++mt) {
#pragma unroll
    for (int i = 0; i < D::CL; ++i) {
      const int idx = tid + 256 * i;
      const int o = (idx / D::CPR) * D::RS + (idx % D::CPR) * 16;
      *reinterpret_cast<u32x4*>(xs + o) = xr[i];
      *reinterpret_cast<u32x4*>(ys + o) = yr[i];
    }
    __syncthreads();
    if (mt + 1 < nmt) {   // workgroup-uniform
#pragma unroll
      for (int i = 0; i < D::CL; ++i) {
        xr[i] = xty_chunk<T>(X, a.ldx, k0, a.Kmem, (mt + 1) * XRM, rows, tid + 256 * i);
        yr[i] = xty_chunk<T>(Y, a.ldy, n0, a.N, (mt + 1) * XRM, rows, tid + 256 * i);
      }
    }
    xty_mma(xs, ys, wk, wn, fr, fg, acc, (T*)nullptr);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int k = k0 + wk * 32 + i * 16 + fr;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 32 + j * 16 + 4 * fg;
      if (k < a.K && n < a.N) *reinterpret_cast<f32x4*>(C + (long)k * a.ldc + n) = acc[i][j];
    }
  }
}

// grid B, 256 threads.  xn [B*T][D]: the final LayerNorm of the CLS rows.  pooled as vcap_vit_head_kernel sums
// it (frames w, w + 4, ... per partial, partials in order); dn [B*T][D] = (grad_out[b] . proj_w) / T
__global__ __launch_bounds__(256) void vcap_vit_head_bwd_kernel(const float* __restrict__ xn, int T, int D,
                                                                const float* __restrict__ gout,
                                                                const float* __restrict__ pw, int VD,
                                                                float* __restrict__ pooled, float* __restrict__ dn) {
  const int b = blockIdx.x;
  for (int c = threadIdx.x; c < D; c += 256) {
    float part[4] = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < T; ++t) part[t & 3] += xn[((long)b * T + t) * D + c];
    pooled[(long)b * D + c] = (part[0] + part[1] + part[2] + part[3]) / (float)T;
    float acc = 0.f;
    for (int v = 0; v < VD; ++v) acc = fmaf(gout[(long)b * VD + v], pw[(long)v * D + c], acc);
    const float d = acc / (float)T + 0.f;
    for (int t = 0; t < T; ++t) dn[((long)b * T + t) * D + c] = d;
  }
}

// grid VD, 256 threads: row v of encoder.proj's dW, videos in order; thread 0 also sums db[v]
__global__ __launch_bounds__(256) void vcap_vit_proj_grad_kernel(const float* __restrict__ gout,
                                                                 const float* __restrict__ pooled, int B, int D,
                                                                 int VD, float* __restrict__ dw,
                                                                 float* __restrict__ db) {
  const int v = blockIdx.x;
  for (int c = threadIdx.x; c < D; c += 256) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc = fmaf(gout[(long)b * VD + v], pooled[(long)b * D + c], acc);
    dw[(long)v * D + c] = acc;
  }
  if (threadIdx.x == 0) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc += gout[(long)b * VD + v];
    db[v] = acc;
  }
}

// grid N, 256 threads: dpos[n][c] = sum over the BT frames in order of g[bt * N + n][c]; row 0 is also dcls
__global__ __launch_bounds__(256) void vcap_vit_pos_grad_kernel(const float* __restrict__ g, int BT, int N, int D,
                                                                float* __restrict__ dpos, float* __restrict__ dcls) {
  const int n = blockIdx.x;
  for (int c = threadIdx.x; c < D; c += 256) {
    float acc = 0.f;
    for (int bt = 0; bt < BT; ++bt) acc += g[((long)bt * N + n) * D + c];
    dpos[(long)n * D + c] = acc;
    if (n == 0) dcls[c] = acc;
  }
}

// grid rows, 256 threads: dst[r * ldd + i] = src[r * lds + i], i < width
__global__ __launch_bounds__(256) void vcap_vit_rows_copy_kernel(const float* __restrict__ src, long lds,
                                                                 float* __restrict__ dst, long ldd, long width) {
  const float* s = src + (long)blockIdx.x * lds;
  float* d = dst + (long)blockIdx.x * ldd;
  for (long i = threadIdx.x; i < width; i += 256) d[i] = s[i];
}

// ---- dispatchers ------------------------------------------------------------------------------------
int vcap_vit_attn_bwd_ldp(int N) { return (N + 63) / 64 * 64; }

hipError_t vcap_vit_xty_dispatch(int dt, const XtyArgs& a, int Z, hipStream_t s) {
  const long es = (long)vcap_dt_size(dt), epc = 16 / (es ? es : 1);
  if ((dt != VCAP_DT_F32 && dt != VCAP_DT_BF16) || a.K <= 0 || a.N <= 0 || Z <= 0 || a.Z2 <= 0 || a.rows_total <= 0 ||
      a.slab_rows <= 0 || Z > 65535 || a.Kmem < a.K || a.Kmem % epc || a.N % epc || a.N % 4 || a.ldx % epc || a.ldy % epc ||
      a.ldx < a.Kmem || a.ldy < a.N || a.ldc % 4 || a.xs1 % epc || a.xs2 % epc || a.ys1 % epc || a.ys2 % epc ||
      a.cs1 % 4 || a.cs2 % 4 || ((uintptr_t)a.X & 15) || ((uintptr_t)a.Y & 15) || ((uintptr_t)a.C & 15) || !a.X ||
      !a.Y || !a.C)
    return hipErrorInvalidValue;
  const dim3 grid((a.K + XT - 1) / XT, (a.N + XT - 1) / XT, Z), block(256);
  if (dt == VCAP_DT_BF16)
    hipLaunchKernelGGL(vcap_vit_xty_kernel<bf16_t>, grid, block, 0, s, a);
  else
    hipLaunchKernelGGL(vcap_vit_xty_kernel<float>, grid, block, 0, s, a);
  return hipGetLastError();
}

hipError_t vcap_vit_attn_bwd_dispatch(int dt, const void* qkv, const void* dO, int BT, int N, int H, void* P, void* dS,
                                      void* dST, float* dqkv, hipStream_t s) {
  if ((dt != VCAP_DT_F32 && dt != VCAP_DT_BF16) || BT <= 0 || H <= 0 || (long)BT * H > 65535 || N < 1 || N > 288 ||
      ((uintptr_t)qkv & 15) ||
      ((uintptr_t)dO & 15) || ((uintptr_t)P & 15) || ((uintptr_t)dS & 15) || ((uintptr_t)dST & 15) ||
      ((uintptr_t)dqkv & 15))
    return hipErrorInvalidValue;
  const int ldp = vcap_vit_attn_bwd_ldp(N), D = 64 * H;
  const dim3 grid((N + 63) / 64, BT * H), block(256);
  if (dt == VCAP_DT_BF16)
    hipLaunchKernelGGL(vcap_vit_attn_bwd_probs_kernel<bf16_t>, grid, block, 0, s, (const bf16_t*)qkv,
                       (const bf16_t*)dO, N, H, ldp, (bf16_t*)P, (bf16_t*)dS, (bf16_t*)dST);
  else
    hipLaunchKernelGGL(vcap_vit_attn_bwd_probs_kernel<float>, grid, block, 0, s, (const float*)qkv, (const float*)dO,
                       N, H, ldp, (float*)P, (float*)dS, (float*)dST);
  if (hipError_t e = hipGetLastError()) return e;
  const size_t es = vcap_dt_size(dt);
  // dQ = (dS^T)^T K, dK = dS^T Q, dV = P^T dO per (frame, head): rows = the contracted tokens
  const void* xs[3] = {dST, dS, P};
  const char* q = (const char*)qkv;
  const void* ys[3] = {q + (size_t)D * es, q, dO};
  const long ldy[3] = {3L * D, 3L * D, D};
  for (int i = 0; i < 3; ++i) {
    XtyArgs a{};
    a.X = xs[i];
    a.ldx = ldp;
    a.Kmem = ldp;
    a.Y = ys[i];
    a.ldy = ldy[i];
    a.N = 64;
    a.C = dqkv + (long)i * D;
    a.ldc = 3L * D;
    a.K = N;
    a.rows_total = N;
    a.slab_rows = N;
    a.slab_step = 0;
    a.Z2 = H;
    a.xs1 = (long)H * ldp * ldp;
    a.xs2 = (long)ldp * ldp;
    a.ys1 = (long)N * ldy[i];
    a.ys2 = 64;
    a.cs1 = (long)N * 3 * D;
    a.cs2 = 64;
    if (hipError_t e = vcap_vit_xty_dispatch(dt, a, BT * H, s)) return e;
  }
  return hipSuccess;
}

hipError_t vcap_vit_head_bwd_dispatch(const float* xn, int B, int T, int D, const float* gout, const float* pw, int VD,
                                      float* pooled, float* dn, float* dproj_w, float* dproj_b, hipStream_t s) {
  if (B <= 0 || T <= 0 || D <= 0 || VD <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vcap_vit_head_bwd_kernel, dim3(B), dim3(256), 0, s, xn, T, D, gout, pw, VD, pooled, dn);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(vcap_vit_proj_grad_kernel, dim3(VD), dim3(256), 0, s, gout, (const float*)pooled, B, D, VD,
                     dproj_w, dproj_b);
  return hipGetLastError();
}

hipError_t vcap_vit_pos_grad_dispatch(const float* g, int BT, int N, int D, float* dpos, float* dcls, hipStream_t s) {
  if (BT <= 0 || N <= 0 || D <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vcap_vit_pos_grad_kernel, dim3(N), dim3(256), 0, s, g, BT, N, D, dpos, dcls);
  return hipGetLastError();
}

hipError_t vcap_vit_rows_copy_dispatch(const float* src, long lds, float* dst, long ldd, int rows, long width,
                                       hipStream_t s) {
  if (rows <= 0 || width <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vcap_vit_rows_copy_kernel, dim3(rows), dim3(256), 0, s, src, lds, dst, ldd, width);
  return hipGetLastError();
}
