// The weight-gradient product of vcap_gpt2_score_backward_tail (schedule: runtime_gpt2_grad.hip):
//
//   vcap_gpt2_dw_kernel<T>      dW[k][n] = sum_{m < M} X[m][k] dY[m][n], X [M][K] and dY [M][N] row-major in the
//                               decoder dtype T read from HBM as they lie, dW f32 [K][N] row-major (HF's Conv1D
//                               [in, out], the parameter's own layout).  K % 64 == 0, N % 128 == 0, 1 <= M <= 512.
//
// One workgroup of 4 waves (2 x 2) owns a 64 (k) x 128 (n) output tile - a constant, so the grid is a function
// of (K, N) alone - and walks ALL M rows in ascending 32-row tiles: no split of the row axis, no slabs, no
// atomics, no second launch.  One wave sums each output element, so the order of a sum over m is the row
// order whatever M is, and rows whose dY is zero add exactly nothing.
//
// Per row tile the [32][64] piece of X and the [32][128] piece of dY go HBM -> registers -> LDS as 16-byte
// chunks, row-major.  Rows at and past M are part of the reduction (unlike gemm_tile.h's output rows, which
// may re-read the last row), so their chunks are literal zeros: the register stage writes (0, 0, 0, 0)
// instead of loading.  The next tile's global loads are issued before the current tile's MFMAs.
//
// Both MFMA operands have the reduction index m as their k axis, i.e. they are COLUMNS of the row-major LDS
// images:
//   bf16 (16x16x32): lane (fr = lane & 15, fg = lane >> 4) needs rows 8 fg .. 8 fg + 7 of column c0 + fr: two
//     ds_read_b64_tr_b16 (rows 8 fg + 0..3 and + 4..7).  Within a 16-lane group, lane 4 q + p supplies the
//     address of row q, columns c0 + 4 p .. + 3 (8 bytes, 8-byte aligned: the row strides are multiples of 16).
//     Every lane of every wave executes every read (EXEC all ones): there is no early exit and the padding
//     rows exist in LDS as zeros.
//   f32 (16x16x4): step s of 8 needs the one element [4 s + fg][c0 + fr]: a plain ds_read_b32.
// X and dY are read through the same address function, so slot (fg, j) of both operands is the same row m.
// acc = mfma(a = dY fragment, b = X fragment): lane (fr, fg) holds dW[k0 + fr][n0 + 4 fg + e], e < 4 - four
// consecutive columns of one row, stored as one float4.
//
// Row strides carry 16 (bf16) / 64 (f32) bytes of padding: 16-byte aligned for the chunk stores; for f32 the
// stride is 16 banks mod 32, so the two rows a 32-lane half reads are on disjoint banks.
//
// Exact zeros: accumulators start at +0 and only add; a product with a +-0 factor is +-0 and +0 + -0 = +0.
#include "vcap_common.h"
#include "vcap_kernels.h"

namespace {

constexpr int TK = 64, TN = 128, RM = 32;   // output tile (X columns x dY columns), rows per reduction step

template <typename T>
struct DwTile {
  static constexpr int PAD = sizeof(T) == 2 ? 16 : 64;
  static constexpr int XS = TK * (int)sizeof(T) + PAD;   // row strides of the two LDS images, bytes
  static constexpr int YS = TN * (int)sizeof(T) + PAD;
  static constexpr int XB = RM * XS, YB = RM * YS;
  static constexpr int EPC = 16 / (int)sizeof(T);        // elements per 16-byte chunk
  static constexpr int XCPR = TK / EPC, YCPR = TN / EPC;  // chunks per image row
  static constexpr int XL = RM * XCPR / 256, YL = RM * YCPR / 256;   // chunks per thread
};

// chunk i of this thread of a [RM][cols] tile whose first row is m0: rows >= M are zeros
template <typename T, int CPR>
VCAP_DEV u32x4 load_chunk(const T* __restrict__ P, long ld, int col0, int m0, int M, int idx) {
  const int r = idx / CPR, ch = idx % CPR;
  const int m = m0 + r;
  if (m >= M) return (u32x4){0u, 0u, 0u, 0u};
  return *reinterpret_cast<const u32x4*>(P + (long)m * ld + col0 + ch * (16 / (int)sizeof(T)));
}

VCAP_DEV u32x2 tr_read16(const char* p) {
  typedef __attribute__((ext_vector_type(4))) short s16x4;
  const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
  return __builtin_bit_cast(u32x2, v);
}

// rows 8 fg .. 8 fg + 7 of column c0 + fr of a row-major bf16 image
VCAP_DEV u32x4 col_frag16(const char* img, int stride, int c0, int fr, int fg) {
  const char* p = img + (8 * fg + (fr >> 2)) * stride + (c0 + 4 * (fr & 3)) * 2;
  const u32x2 lo = tr_read16(p), hi = tr_read16(p + 4 * stride);
  return (u32x4){lo.x, lo.y, hi.x, hi.y};
}

// the 32 staged rows of both images into the wave's 2 x 4 accumulators
VCAP_DEV void dw_tile_mma(const char* xs, const char* ys, int wk, int wn, int fr, int fg, f32x4 (&acc)[2][4],
                          bf16_t*) {
  typedef DwTile<bf16_t> D;
  u32x4 xf[2], yf[4];
#pragma unroll
  for (int i = 0; i < 2; ++i) xf[i] = col_frag16(xs, D::XS, wk * 32 + i * 16, fr, fg);
#pragma unroll
  for (int j = 0; j < 4; ++j) yf[j] = col_frag16(ys, D::YS, wn * 64 + j * 16, fr, fg);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = mfma_frag(yf[j], xf[i], acc[i][j], (bf16_t*)nullptr);
}

VCAP_DEV void dw_tile_mma(const char* xs, const char* ys, int wk, int wn, int fr, int fg, f32x4 (&acc)[2][4],
                          float*) {
  typedef DwTile<float> D;
#pragma unroll
  for (int s = 0; s < RM / 4; ++s) {
    const int r = 4 * s + fg;
    float xv[2], yv[4];
#pragma unroll
    for (int i = 0; i < 2; ++i) xv[i] = *reinterpret_cast<const float*>(xs + r * D::XS + (wk * 32 + i * 16 + fr) * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) yv[j] = *reinterpret_cast<const float*>(ys + r * D::YS + (wn * 64 + j * 16 + fr) * 4);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[j], xv[i], acc[i][j], 0, 0, 0);
  }
}

}  // namespace

// grid (N / 128, K / 64), 256 threads
template <typename T>
__global__ __launch_bounds__(256) void vcap_gpt2_dw_kernel(const T* __restrict__ X, const T* __restrict__ dY,
                                                           float* __restrict__ dW, int M, int K, int N) {
  typedef DwTile<T> D;
  __shared__ __attribute__((aligned(16))) char smem[D::XB + D::YB];
  char* xs = smem;
  char* ys = smem + D::XB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wk = wave >> 1, wn = wave & 1, fr = lane & 15, fg = lane >> 4;
  const int n0 = blockIdx.x * TN, k0 = blockIdx.y * TK;
  f32x4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  u32x4 xr[D::XL], yr[D::YL];
#pragma unroll
  for (int i = 0; i < D::XL; ++i) xr[i] = load_chunk<T, D::XCPR>(X, K, k0, 0, M, tid + 256 * i);
#pragma unroll
  for (int i = 0; i < D::YL; ++i) yr[i] = load_chunk<T, D::YCPR>(dY, N, n0, 0, M, tid + 256 * i);
  const int nmt = (M + RM - 1) / RM;
  for (int mt = 0; mt < nmt; ++mt) {
#pragma unroll
    for (int i = 0; i < D::XL; ++i) {
      const int idx = tid + 256 * i;
      *reinterpret_cast<u32x4*>(xs + (idx / D::XCPR) * D::XS + (idx % D::XCPR) * 16) = xr[i];
    }
#pragma unroll
    for (int i = 0; i < D::YL; ++i) {
      const int idx = tid + 256 * i;
      *reinterpret_cast<u32x4*>(ys + (idx / D::YCPR) * D::YS + (idx % D::YCPR) * 16) = yr[i];
    }
    __syncthreads();
    if (mt + 1 < nmt) {   // workgroup-uniform
#pragma unroll
      for (int i = 0; i < D::XL; ++i) xr[i] = load_chunk<T, D::XCPR>(X, K, k0, (mt + 1) * RM, M, tid + 256 * i);
#pragma unroll
      for (int i = 0; i < D::YL; ++i) yr[i] = load_chunk<T, D::YCPR>(dY, N, n0, (mt + 1) * RM, M, tid + 256 * i);
    }
    dw_tile_mma(xs, ys, wk, wn, fr, fg, acc, (T*)nullptr);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long k = k0 + wk * 32 + i * 16 + fr;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<f32x4*>(dW + k * N + n0 + wn * 64 + j * 16 + 4 * fg) = acc[i][j];
  }
}

hipError_t vcap_gpt2_dw_dispatch(int dt, const void* X, const void* dY, float* dW, int M, int K, int N,
                                 hipStream_t s) {
  if (M <= 0 || M > 512 || K <= 0 || K % TK || N <= 0 || N % TN || !X || !dY || !dW || ((uintptr_t)X & 15) ||
      ((uintptr_t)dY & 15) || ((uintptr_t)dW & 15))
    return hipErrorInvalidValue;
  const dim3 grid(N / TN, K / TK), block(256);
  if (dt == VCAP_DT_BF16)
    hipLaunchKernelGGL(vcap_gpt2_dw_kernel<bf16_t>, grid, block, 0, s, (const bf16_t*)X, (const bf16_t*)dY, dW, M, K, N);
  else if (dt == VCAP_DT_F32)
    hipLaunchKernelGGL(vcap_gpt2_dw_kernel<float>, grid, block, 0, s, (const float*)X, (const float*)dY, dW, M, K, N);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}
