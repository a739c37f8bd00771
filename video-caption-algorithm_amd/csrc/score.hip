// Teacher-forced scoring (vcap_gpt2_score): the tied lm_head and the cross-entropy over EVERY row of a
// prefix + caption forward, where the decode kernels (decode.hip) only ever score each sequence's
// last row.  Replaces GPT2LMHeadModel's lm_head + CrossEntropyLoss(ignore_index=-100) as the
// reference's teacher-forced entry points reach it (src/models/text_decoder.py:76-103,
// src/models/caption_model.py:104-168).
//
//   logits[m][v] = xn[m] . wte[v]      xn = ln_f(h), rounded to the decoder dtype where PRO_LN rounds it
//   logprob[m]   = logits[m][target[m]] - log sum_v exp(logits[m][v])
//
// vcap_score_lm_kernel: one workgroup per 128-column tile of the vocabulary, walking all row tiles
// (<= 4: vcap_gpt2_max_rows() rows) with the 128x128 MFMA tile loop of the ViT GEMM (gemm_tile.h)
// against plain wte ([V, E] is that loop's W layout in both dtypes).  The tile's weights come from HBM
// once: the second to fourth row tiles of the same workgroup re-read them through the cache
// hierarchy moments later.  [M, V] logits are stored only on request (STORE); what every call keeps is,
// per (row, 64-column part = one wave's half of the tile), the part's max and sum exp(x - max), plus
// the target's logit from the one part that holds its column.  Columns past V (the last tile of
// 50257 = 392 * 128 + 81 holds 81 real columns) enter neither; rows past M write nothing.
// vcap_score_combine_kernel merges a row's parts in part order, vcap_score_loss_kernel adds the rows
// in row order: fixed orders, no float atomics, so two calls give the same bits.
#include "gemm_tile.h"
#include "vcap_common.h"
#include "vcap_kernels.h"

using namespace gemm_tile;

template <typename T, bool STORE>
__global__ __launch_bounds__(256) void vcap_score_lm_kernel(const T* __restrict__ A, const T* __restrict__ W, int M,
                                                            int V, int K, const int* __restrict__ targets,
                                                            float* __restrict__ logits, float* __restrict__ part_max,
                                                            float* __restrict__ part_sum,
                                                            float* __restrict__ tgt_logit, int nparts) {
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_BYTES];
  static_assert(!STORE || BM * BN * sizeof(float) <= 2 * STAGE_BYTES, "the f32 tile is staged through smem");
  constexpr int BK = ROWB / sizeof(T);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, fr = lane & 15, fg = lane >> 4;
  const int n0 = blockIdx.x * BN;
  const int cb = n0 + wn * 64 + 4 * fg;  // this lane's first column; + j * 16 + e
  const int part = blockIdx.x * 2 + wn;

  for (int m0 = 0; m0 < M; m0 += BM) {
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    tile_loop(A, (long)K, W, (long)K, m0, M, n0, V, 0, K / BK, smem, acc);

#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + wm * 64 + i * 16 + fr;
      const int tgt = targets ? targets[min(m, M - 1)] : -1;
      float mx = -INFINITY, tv = 0.f;
      bool hit = false;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = cb + j * 16 + e;
          if (col < V) mx = fmaxf(mx, acc[i][j][e]);
          if (col == tgt) {  // tgt in [0, V): a real column, held by exactly one lane of the grid
            tv = acc[i][j][e];
            hit = true;
          }
        }
      mx = rows_max(mx);  // the row's 64 columns of this part sit in lanes fr, fr + 16, fr + 32, fr + 48
      const float base = mx == -INFINITY ? 0.f : mx;  // a part past V: sum 0, max -inf
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (cb + j * 16 + e < V) sum += __expf(acc[i][j][e] - base);
      sum = rows_sum(sum);
      if (m < M) {
        if (fg == 0) {
          part_max[(long)m * nparts + part] = mx;
          part_sum[(long)m * nparts + part] = sum;
        }
        if (hit) tgt_logit[m] = tv;
      }
    }

    if constexpr (STORE) {
      // tile -> LDS -> rows of 128 consecutive columns: 512-byte runs per row (V is odd, so a lane's
      // 4 columns are not 16-byte aligned in logits; a direct store would write 16 rows x 16 bytes)
      float* st = reinterpret_cast<float*>(smem);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          *reinterpret_cast<f32x4*>(st + (wm * 64 + i * 16 + fr) * BN + wn * 64 + j * 16 + 4 * fg) = acc[i][j];
      __syncthreads();
      for (int r = wave; r < BM; r += 4) {
        const int m = m0 + r;
        if (m >= M) break;
#pragma unroll
        for (int c = lane; c < BN; c += 64)
          if (n0 + c < V) logits[(long)m * V + n0 + c] = st[r * BN + c];
      }
      __syncthreads();  // the next row tile stages into smem
    }
  }
}

// One wave per row: the row's parts merged in a fixed order (lane p, p + 64, ... online, then one
// butterfly over the lanes), logprob = target logit - (max + log sum).
__global__ __launch_bounds__(256) void vcap_score_combine_kernel(const float* __restrict__ part_max,
                                                                 const float* __restrict__ part_sum, int nparts,
                                                                 const float* __restrict__ tgt_logit,
                                                                 const int* __restrict__ targets,
                                                                 const uint8_t* __restrict__ kmask, int S, int V, int M,
                                                                 float* __restrict__ logprob_ws,
                                                                 float* __restrict__ logprob_out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  float mx = -INFINITY, sum = 0.f;
  for (int p = lane; p < nparts; p += 64) {
    const float pm = part_max[(long)row * nparts + p], ps = part_sum[(long)row * nparts + p];
    if (pm > mx) {
      sum = sum * expf(mx - pm) + ps;  // mx = -inf: sum is 0
      mx = pm;
    } else if (pm != -INFINITY) {
      sum += ps * expf(pm - mx);
    }
  }
  const float gm = wave_max(mx);  // finite: part 0 holds real columns
  const float tot = wave_sum(mx == -INFINITY ? 0.f : sum * expf(mx - gm));
  const int tgt = targets[row];
  float lp = (tgt >= 0 && tgt < V) ? tgt_logit[row] - (gm + logf(tot)) : 0.f;
  // a sequence whose first key is hidden breaks the call's precondition: poison its rows
  if (kmask && kmask[(long)(row / S) * S] == 0) lp = __builtin_nanf("");
  if (lane == 0) {
    logprob_ws[row] = lp;
    if (logprob_out) logprob_out[row] = lp;
  }
}

// loss_out = {sum of -logprob over the counted rows, count}: thread t adds rows t, t + 256, ... in
// order, then a fixed tree over the 256 threads.
__global__ __launch_bounds__(256) void vcap_score_loss_kernel(const float* __restrict__ logprob_ws,
                                                              const int* __restrict__ targets, int V, int M,
                                                              float* __restrict__ loss_out) {
  __shared__ float s_sum[256];
  __shared__ float s_cnt[256];
  const int tid = threadIdx.x;
  float sum = 0.f, cnt = 0.f;
  for (int r = tid; r < M; r += 256) {
    const int tgt = targets[r];
    if (tgt >= 0 && tgt < V) {
      sum -= logprob_ws[r];
      cnt += 1.f;
    }
  }
  s_sum[tid] = sum;
  s_cnt[tid] = cnt;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      s_sum[tid] += s_sum[tid + w];
      s_cnt[tid] += s_cnt[tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    loss_out[0] = s_sum[0];
    loss_out[1] = s_cnt[0];
  }
}

int vcap_score_parts(int V) { return 2 * ((V + BN - 1) / BN); }

template <typename T>
static hipError_t launch_score_lm(const ScoreLmArgs& a, hipStream_t s) {
  const dim3 grid((a.V + BN - 1) / BN), block(256);
  if (a.logits)
    hipLaunchKernelGGL((vcap_score_lm_kernel<T, true>), grid, block, 0, s, (const T*)a.xn, (const T*)a.wte, a.M, a.V,
                       a.E, a.targets, a.logits, a.part_max, a.part_sum, a.tgt_logit, a.nparts);
  else
    hipLaunchKernelGGL((vcap_score_lm_kernel<T, false>), grid, block, 0, s, (const T*)a.xn, (const T*)a.wte, a.M, a.V,
                       a.E, a.targets, a.logits, a.part_max, a.part_sum, a.tgt_logit, a.nparts);
  return hipGetLastError();
}

hipError_t vcap_score_lm_dispatch(int dt, const ScoreLmArgs& a, hipStream_t s) {
  const int bk = ROWB / (int)vcap_dt_size(dt);
  if (a.M <= 0 || a.V <= 0 || a.E <= 0 || a.E % bk || a.nparts != vcap_score_parts(a.V) ||
      ((uintptr_t)a.xn & 15) || ((uintptr_t)a.wte & 15))
    return hipErrorInvalidValue;
  if (dt == VCAP_DT_BF16) return launch_score_lm<bf16_t>(a, s);
  if (dt == VCAP_DT_F32) return launch_score_lm<float>(a, s);
  return hipErrorInvalidValue;
}

hipError_t vcap_score_combine_dispatch(const ScoreLmArgs& a, const uint8_t* kmask, int S, float* logprob_ws,
                                       float* logprob_out, float* loss_out, hipStream_t s) {
  if (!a.targets || !logprob_ws || S <= 0 || a.M % S) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vcap_score_combine_kernel, dim3((a.M + 3) / 4), dim3(256), 0, s, (const float*)a.part_max,
                     (const float*)a.part_sum, a.nparts, (const float*)a.tgt_logit, a.targets, kmask, S, a.V, a.M,
                     logprob_ws, logprob_out);
  if (hipError_t e = hipGetLastError()) return e;
  if (loss_out)
    hipLaunchKernelGGL(vcap_score_loss_kernel, dim3(1), dim3(256), 0, s, (const float*)logprob_ws, a.targets, a.V, a.M,
                       loss_out);
  return hipGetLastError();
}
