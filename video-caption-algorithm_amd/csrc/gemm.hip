// Tiled MFMA GEMM for the ViT hot loop (patch-embed, QKV, attn-proj, fc1, fc2) and the
// prefix mapper:  C[M,N] = epilogue( A[M,K] . W[N,K]^T ).
//
// Replaces the reference's Linear layers inside timm Block/Attention/Mlp
// (src/models/video_encoder.py:162-172 patched forward; GELU forced to tanh at :123-134)
// and the CuPy `linear_bias_f32/_f16` kernels (core/operators/cupy_linear_mapper.py:14-70):
// W keeps torch Linear's [out, in] row-major layout, so both operands are K-contiguous.
//
// Tile 128x128, 256 threads = 4 waves in 2x2, each wave 64x64 = 4x4 MFMA 16x16 tiles.
// K step = 128 bytes per row (64 bf16 or 32 f32).  Operands stream global->LDS with
// global_load_lds_dwordx4 (1 KiB per wave instruction, lane-linear LDS image); the
// st_8x16B XOR swizzle (chunk ^ (row & 7)) is applied on the global SOURCE address and on
// the ds_read address, making the ds_read_b128 fragment reads conflict-free.
// bf16 / f16 use mfma_f32_16x16x32_bf16 / _f16 (f16: the reference's autocast dtype, rounded where
// autocast rounds: Autocast<T> in vcap_common.h); the fp32 parity mode uses mfma_f32_16x16x4f32 with the
// SAME byte layout (one 16-byte chunk = 4 f32 = one group of four 16x16x4 MFMAs).
#include "gemm_tile.h"
#include "vcap_common.h"
#include "vcap_kernels.h"

using namespace gemm_tile;

// EPI (compile time, so each ViT GEMM role is its own kernel symbol in a profile):
//   0 bias (QKV)   1 bias+gelu_tanh (fc1)   2 bias+residual in place (attn-proj, fc2)
//   3 general: runtime act / residual mode / row remap (patch-embed, vcap_gemm ABI)
template <typename TIn, typename TOut, int EPI>
__global__ __launch_bounds__(256) void vcap_gemm_kernel(const TIn* __restrict__ A, long lda,
                                                        const TIn* __restrict__ W, long ldw,
                                                        TOut* C, long ldc, int M, int N, int K, GemmEpi epi) {
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_BYTES];
  constexpr int BK = ROWB / sizeof(TIn);

  const int tiles_n = (N + BN - 1) / BN;
  const int tiles_m = (M + BM - 1) / BM;
  const int nwg = tiles_m * tiles_n;
  // XCD-aware bijective remap: blocks b, b+8, ... share an XCD; give each XCD a contiguous run
  // of tile ids so its L2 sees the same A row-panel across consecutive N tiles.
  const int bid = blockIdx.x;
  const int xcd = bid & 7, q = nwg >> 3, r8 = nwg & 7;
  const int wgid = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + (bid >> 3);
  const int tm = wgid / tiles_n, tn = wgid % tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // split-K (gridDim.y > 1): this workgroup sums K-tiles [kt0, kt0 + nk) and stores its partial
  // tile into slab blockIdx.y of epi.splitk_ws; vcap_splitk_reduce_kernel adds the slabs in split
  // order (deterministic: the same sum on every run and on every stream's CU mask)
  const int nk = K / BK / (int)gridDim.y;
  const int kt0 = (int)blockIdx.y * nk;
  const bool split = gridDim.y > 1;
  tile_loop(A, lda, W, ldw, m0, M, n0, N, kt0, nk, smem, acc);
  const int fr = lane & 15, fg = lane >> 4;

  // epilogue: lane holds row fr, columns 4*fg .. 4*fg+3 of each 16x16 tile.  The vector branch asks for whole
  // 16-byte vectors per row (N, ldc, ldr), not for 16-byte aligned C / residual pointers: its f32x4 / u32x2
  // accesses are plain global loads and stores, which the device serves at the element's alignment (unaligned
  // access mode, the HSA default; only the operands' LDS-DMA needs 16 bytes - vcap_gemm checks those).
  const bool vec = (N & 3) == 0 && (ldc & 3) == 0 && (!epi.res || (epi.ldr & 3) == 0);
  // in-place residual (EPI 2): every residual row of the wave is loaded before the first store
  // (load / add / store per element serialised 16 HBM round trips: the loads cannot pass the
  // previous store to the same pointer, and the in-order vmcnt waits for that store too)
  f32x4 rpre[4][4];
  const bool pre = EPI == 2 && vec && !split;
  if constexpr (EPI == 2) {
    if (pre) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = min(m0 + wm * 64 + i * 16 + fr, M - 1);
          const int nb = min(n0 + wn * 64 + j * 16 + 4 * fg, N - 4);
          rpre[i][j] = *reinterpret_cast<const f32x4*>(epi.res + (long)m * epi.ldr + nb);
        }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int nb = n0 + wn * 64 + j * 16 + 4 * fg;
    if (nb >= N) continue;
    float bias[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) bias[e] = (epi.bias && nb + e < N && !split) ? epi.bias[nb + e] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + wm * 64 + i * 16 + fr;
      if (m >= M) continue;
      long orow = m;
      if constexpr (EPI == 3) orow = epi.G ? (long)(m / epi.G) * epi.Gs + epi.goff + (m % epi.G) : (long)m;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = acc[i][j][e] + bias[e];
      // f16 operands: the Linear's output is fp16 under autocast (the split-K sum rounds in its reduce;
      // a plain 16-bit store rounds by itself, and rounding is idempotent)
      if constexpr (Autocast<TIn>::kRound && !(EPI == 0 && sizeof(TOut) == 2)) {
        if (!split)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = Autocast<TIn>::rnd(v[e]);
      }
      if (split) {  // raw partial sums (N % 4 == 0: dispatcher)
        *reinterpret_cast<f32x4*>(epi.splitk_ws + ((long)blockIdx.y * M + m) * N + nb) = (f32x4){v[0], v[1], v[2], v[3]};
        continue;
      }
      // The GELU's output is rounded by the 16-bit store itself (the packed f32x2 conversion: the
      // product is rounded to f32, then to f16, in both GEMM kernels; a scalar conversion here could be
      // contracted with the GELU's last multiply into one v_fma_mixlo_f16, which rounds once and would
      // differ from the 256x256 kernel at f16 ties).  Only an f32 output needs the explicit rounding.
      if constexpr (EPI == 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = gelu_tanh(v[e]);
      } else if constexpr (EPI == 3) {
        if (epi.act == 1)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = sizeof(TOut) == 4 ? Autocast<TIn>::rnd(gelu_tanh(v[e])) : gelu_tanh(v[e]);
      }
      const float* rr = nullptr;
      if constexpr (EPI == 2) rr = epi.res + orow * epi.ldr + nb;
      if constexpr (EPI == 3) {
        if (epi.res_mode == 1) rr = epi.res + orow * epi.ldr + nb;
        else if (epi.res_mode == 2) rr = epi.res + (long)((m % epi.G) + epi.roff) * epi.ldr + nb;
      }
      if (vec && nb + 3 < N) {
        if (pre) {
          const f32x4 r = rpre[i][j];
          v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
        } else if (rr) {
          const f32x4 r = *reinterpret_cast<const f32x4*>(rr);
          v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
        }
        if constexpr (sizeof(TOut) == 2) {
          *reinterpret_cast<u32x2*>(C + orow * ldc + nb) =
              (u32x2){Pack2<TOut>::pack(v[0], v[1]), Pack2<TOut>::pack(v[2], v[3])};
        } else {
          *reinterpret_cast<f32x4*>(C + orow * ldc + nb) = (f32x4){v[0], v[1], v[2], v[3]};
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (nb + e >= N) continue;
          C[orow * ldc + nb + e] = Num<TOut>::from_f(v[e] + (rr ? rr[e] : 0.f));
        }
      }
    }
  }
}

// C[orow(m)][n] = (sum over splits s = 0.. of ws[s][m][n] + bias[n]) + C[orow(m)][n]: the split-K
// partials of an in-place residual GEMM, summed in a fixed order.  R16 (f16 operands): the sum + bias is
// rounded to fp16 before the residual add, where the unsplit epilogue rounds it.
template <bool R16>
__global__ __launch_bounds__(256) void vcap_splitk_reduce_kernel(const float* __restrict__ ws, int splits, float* C,
                                                                 long ldc, int M, int N, GemmEpi epi) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;  // f32x4 index
  const int nq = N >> 2;
  if (i >= (long)M * nq) return;
  const int m = (int)(i / nq), n = (int)(i - (long)m * nq) * 4;
  f32x4 v = *reinterpret_cast<const f32x4*>(ws + (long)m * N + n);
  for (int sp = 1; sp < splits; ++sp) v += *reinterpret_cast<const f32x4*>(ws + ((long)sp * M + m) * N + n);
  if (epi.bias) v += *reinterpret_cast<const f32x4*>(epi.bias + n);
  if constexpr (R16) v = Autocast<f16_t>::rnd4(v);
  const long orow = epi.G ? (long)(m / epi.G) * epi.Gs + epi.goff + (m % epi.G) : (long)m;
  float* c = C + orow * ldc + n;
  *reinterpret_cast<f32x4*>(c) = v + *reinterpret_cast<const f32x4*>(c);
}

// K splits of the latest 128x128 launch issued by this thread (1 = unsplit): vcap_gemm_splitk reports it
static thread_local int g_last_splits = 1;
int vcap_gemm_last_splits() { return g_last_splits; }

// K splits of the 128x128 kernel for one launch (1 = unsplit).
// Few tiles (the CLS-only last block: M = B*T rows) leave most CUs idle through a long K
// loop: split K over several workgroups per tile when C is f32 and already holds the
// residual (attn-proj / fc2 in place) and the caller gave a partials workspace (bf16 / f16 operands
// only: the fp32 parity mode keeps one summation chain).  The split count depends on K alone
// (the largest divisor c <= 8 of the K-tile count leaving >= 3 K-tiles per workgroup), never on
// M or the stream's CU mask, so a row sums the same way whichever batch it is encoded in and a
// CU-masked pipelined encode sums exactly like a serial one.  (No CU-count gate: a large encode
// batch takes more rounds of split workgroups instead of switching the summation order.  The
// encoder's partials workspace holds 16 splits of its B*T CLS rows, so the size check below
// only refuses a caller-supplied workspace that is too small.)
// vcap_gemm_dispatch asks the same function: a launch that splits keeps this kernel under every
// GEMM policy and tile count, because the 256x256 kernel never splits and an unsplit sum is
// another f32 summation order (tests/test_gpu_encoder_shapes.py found the forced 256x256 policy
// changing the last bits of an encode through the CLS tail).
static int gemm_splits(size_t in_size, size_t out_size, const void* C, long ldc, int M, int N, int K,
                       const GemmEpi& epi) {
  if (in_size != 2 || out_size != 4) return 1;
  // launch_gemm gives these launches EPI 2 (plain rows) or EPI 3 (remapped rows), both of which store partials
  const bool in_place = epi.bias != nullptr && epi.res == (const float*)C && epi.ldr == ldc && epi.res_mode == 1 &&
                        epi.act == 0 && epi.splitk_ws && (N & 3) == 0 && (ldc & 3) == 0 && ((uintptr_t)C & 15) == 0;
  if (!in_place) return 1;
  const int nkt = K / (ROWB / 2);
  int c = 1;
  for (int d = 8; d >= 2; --d)
    if (nkt % d == 0 && nkt / d >= 3) {
      c = d;
      break;
    }
  return c > 1 && (size_t)c * M * N * sizeof(float) <= epi.splitk_bytes ? c : 1;
}

template <typename TIn, typename TOut, int EPI>
static hipError_t launch_gemm_epi(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N,
                                  int K, const GemmEpi& epi, hipStream_t s) {
  const int tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  const int splits = (EPI == 2 || EPI == 3) ? gemm_splits(sizeof(TIn), sizeof(TOut), C, ldc, M, N, K, epi) : 1;
  g_last_splits = splits;
  hipLaunchKernelGGL((vcap_gemm_kernel<TIn, TOut, EPI>), dim3(tiles, splits), dim3(256), 0, s, (const TIn*)A, lda,
                     (const TIn*)W, ldw, (TOut*)C, ldc, M, N, K, epi);
  if (splits > 1) {
    if (hipError_t e = hipGetLastError()) return e;
    const long nvec = (long)M * (N / 4);
    hipLaunchKernelGGL(vcap_splitk_reduce_kernel<Autocast<TIn>::kRound>, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, s,
                       (const float*)epi.splitk_ws, splits, (float*)C, ldc, M, N, epi);
  }
  return hipGetLastError();
}

template <typename TIn, typename TOut>
static hipError_t launch_gemm(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N,
                              int K, const GemmEpi& epi, hipStream_t s) {
  const bool plain_rows = epi.G == 0;
  if (plain_rows && epi.res_mode == 0 && epi.act == 0)
    return launch_gemm_epi<TIn, TOut, 0>(A, lda, W, ldw, C, ldc, M, N, K, epi, s);
  if constexpr (sizeof(TOut) == sizeof(TIn)) {
    if (plain_rows && epi.res_mode == 0 && epi.act == 1)
      return launch_gemm_epi<TIn, TOut, 1>(A, lda, W, ldw, C, ldc, M, N, K, epi, s);
  }
  if constexpr (sizeof(TOut) == 4) {
    if (plain_rows && epi.res_mode == 1 && epi.act == 0 && epi.res == (const float*)C && epi.ldr == ldc)
      return launch_gemm_epi<TIn, TOut, 2>(A, lda, W, ldw, C, ldc, M, N, K, epi, s);
  }
  return launch_gemm_epi<TIn, TOut, 3>(A, lda, W, ldw, C, ldc, M, N, K, epi, s);
}

// the 128x128 kernel of an (operand, output) dtype pair: a 2-byte operand type writes itself or f32
static hipError_t launch_gemm_dt(int in_dt, int out_dt, const void* A, long lda, const void* W, long ldw, void* C,
                                 long ldc, int M, int N, int K, const GemmEpi& epi, hipStream_t s) {
  if (in_dt == VCAP_DT_BF16 && out_dt == VCAP_DT_BF16)
    return launch_gemm<bf16_t, bf16_t>(A, lda, W, ldw, C, ldc, M, N, K, epi, s);
  if (in_dt == VCAP_DT_BF16 && out_dt == VCAP_DT_F32)
    return launch_gemm<bf16_t, float>(A, lda, W, ldw, C, ldc, M, N, K, epi, s);
  if (in_dt == VCAP_DT_F16 && out_dt == VCAP_DT_F16)
    return launch_gemm<f16_t, f16_t>(A, lda, W, ldw, C, ldc, M, N, K, epi, s);
  if (in_dt == VCAP_DT_F16 && out_dt == VCAP_DT_F32)
    return launch_gemm<f16_t, float>(A, lda, W, ldw, C, ldc, M, N, K, epi, s);
  if (in_dt == VCAP_DT_F32 && out_dt == VCAP_DT_F32)
    return launch_gemm<float, float>(A, lda, W, ldw, C, ldc, M, N, K, epi, s);
  return hipErrorInvalidValue;
}

static int g_gemm_policy = 0;  // 0 auto, 1 always the 128x128 kernel, 2 the 256x256 kernel where it applies
void vcap_gemm_set_policy(int p) { g_gemm_policy = p; }

int vcap_device_cus() {
  int dev = 0, ncu = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  return ncu;
}

// CUs the stream's kernels may use (hipExtStreamGetCUMask; the encode stream of the overlapped
// pipeline is CU-masked), so the round arithmetic below matches what the stream really gets.
int vcap_stream_cus(hipStream_t s) {
  int dev = 0, ncu = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  uint32_t mask[16] = {0};
  if (hipExtStreamGetCUMask(s, 16, mask) != hipSuccess) return ncu;
  int n = 0;
  for (int i = 0; i < 16; ++i) n += __builtin_popcount(mask[i]);
  return n > 0 && n < ncu ? n : ncu;
}

// in_dt: operand dtype; out_dt: C dtype (the residual stream is f32)
hipError_t vcap_gemm_dispatch(int in_dt, int out_dt, const void* A, long lda, const void* W, long ldw, void* C,
                              long ldc, int M, int N, int K, const GemmEpi& epi, hipStream_t s) {
  g_last_splits = 1;  // the 256x256 kernel never splits
  if (in_dt == VCAP_DT_MXFP8) {  // block-scaled fp8: the 256x256 kernel only
    if (!vcap_gemm256_ok(in_dt, out_dt, lda, ldw, ldc, M, N, K, epi)) return hipErrorInvalidValue;
    return vcap_gemm256_dispatch(in_dt, out_dt, A, lda, W, ldw, C, ldc, M, N, K, epi, s);
  }
  const bool splits = gemm_splits(vcap_dt_size(in_dt), vcap_dt_size(out_dt), C, ldc, M, N, K, epi) > 1;
  if (g_gemm_policy != 1 && !splits && vcap_gemm256_ok(in_dt, out_dt, lda, ldw, ldc, M, N, K, epi)) {
    // 256x256 tiles run one workgroup per CU: they need enough tiles to fill the chip, and a
    // last round that is mostly empty costs a whole tile time.  Rows of the full rounds go to
    // the 256x256 kernel, a small remainder to the 128x128 kernel (2 per CU, one short round).
    const int tn = (N + 255) / 256;
    const long tiles256 = (long)((M + 255) / 256) * tn;
    if (g_gemm_policy == 2) return vcap_gemm256_dispatch(in_dt, out_dt, A, lda, W, ldw, C, ldc, M, N, K, epi, s);
    const int ncu = vcap_stream_cus(s);
    if (tiles256 >= ncu) {
      const long rounds = tiles256 / ncu;
      const long rem = tiles256 - rounds * ncu;
      const bool plain = epi.G == 0 && (epi.res_mode == 0 || epi.res == (const float*)C);
      const int m_full = (int)((rounds * ncu / tn) * 256);  // rows covered by whole 256-tile rounds
      if (plain && rem > 0 && rem * 4 < ncu && m_full > 0 && m_full < M) {
        if (hipError_t e = vcap_gemm256_dispatch(in_dt, out_dt, A, lda, W, ldw, C, ldc, m_full, N, K, epi, s))
          return e;
        const size_t ein = vcap_dt_size(in_dt), eout = vcap_dt_size(out_dt);
        GemmEpi e2 = epi;
        if (epi.res) e2.res = epi.res + (long)m_full * epi.ldr;
        const void* A2 = (const char*)A + (size_t)m_full * lda * ein;
        void* C2 = (char*)C + (size_t)m_full * ldc * eout;
        return launch_gemm_dt(in_dt, out_dt, A2, lda, W, ldw, C2, ldc, M - m_full, N, K, e2, s);
      }
      return vcap_gemm256_dispatch(in_dt, out_dt, A, lda, W, ldw, C, ldc, M, N, K, epi, s);
    }
  }
  return launch_gemm_dt(in_dt, out_dt, A, lda, W, ldw, C, ldc, M, N, K, epi, s);
}

// one 128-byte K-tile row (two for the MXFP8 kernel's paired K-tiles)
int vcap_gemm_k_align(int in_dt) { return in_dt == VCAP_DT_MXFP8 ? 256 : vcap_dt_is16(in_dt) ? 64 : 32; }
