// Video retrieval kernels: L2 normalisation of embedding rows, the f32 -> index storage conversion, and
// the exact flat inner-product top-k search (a scan kernel that reads every database row once and keeps a
// private top-k per workgroup and query, and a merge kernel that selects the final k per query).
//
// Scores.  A 16-row database tile is the A operand and a 16-query tile the B operand of the f32-input
// MFMA (mfma_frag(..., float*): four v_mfma_f32_16x16x4_f32 per 16-byte fragment).  Lane (row l & 15,
// group g = l >> 4) feeds elements [(4 s + g) E, +E) of its row at step s (E = 4 f32 or 8 bf16, one
// 16-byte load), the query fragment holds the same elements, and the instruction sums k = 0..3 (the lane
// groups) in order: the score of (row, query) is one f32 fma chain over a fixed permutation of the
// elements.  It depends on the row, the query, dim and the storage type only - not on the row's index,
// the query's slot, nq, n or the grid.  bf16 rows are widened to f32 in registers (exact); the queries
// stay f32.
//
// Order.  A candidate is one 64-bit key: the score's bits mapped monotonically to an unsigned integer in
// the high word, 0xFFFFFFFF - id in the low word.  key_a > key_b <=> (score_a > score_b) or (equal scores
// and id_a < id_b), so "the k largest keys, descending" is the contract's total order; keys are unique
// because ids are, and 0 is the empty slot (a real key's low word is >= 2^31).  NaN scores get no key.
//
// Top-k.  A workgroup appends every key above its query's threshold (the k-th best it has seen, 0 before
// that) to the query's buffer in the workspace; a slab adds at most kIpSlabRows keys per query, and a
// buffer that could not take another slab is compacted first: all keys ranked by counting (exact, keys
// are unique), the best k kept in order, the threshold raised (in the scan one wave per query, the keys in
// registers; in the merge the workgroup over an LDS copy).  Nothing depends on arrival order, so the
// lists - and after the same procedure in the merge kernel, the output - are a function of the key set.
// No float atomics, no spinning; the only atomics are LDS integer slot counters.
#include "retrieval_common.h"   // the key, compact_topk and the bf16 widening, shared with ivf.hip
#include "vcap_common.h"
#include "vcap_kernels.h"

#include <algorithm>

namespace {

constexpr int kThreads = kIpThreads;
constexpr int kWaveTiles = 2;                                  // 16-row tiles per wave and slab
constexpr int kSlab = (kThreads / 64) * kWaveTiles * 16;       // rows per workgroup step
static_assert(kSlab == kIpSlabRows, "vcap_kernels.h kIpSlabRows");
constexpr int kMergeLoads = 8;                                 // keys per thread and merge round
constexpr int kMergeCap = kIpMaxK + 2 * kThreads;

// compact_topk's selection by ONE wave with the keys in registers (the scan kernel: each wave of the workgroup
// compacts other queries' buffers at once, with no workgroup barrier inside).  buf holds m <= kScanRoom keys
// (m wave-uniform); lane l owns keys l, l + 64, ...; every key is broadcast with v_readlane and each lane
// counts, per key it owns, the keys above it.  All loads of buf precede the first store (the ranks depend on
// every lane's keys).  The caller puts workgroup barriers around the compaction phase.
constexpr int kScanRoom = kIpMaxK + 2 * kSlab;
constexpr int kOwn = kScanRoom / 64;
static_assert(kScanRoom % 64 == 0, "whole registers of keys");
VCAP_DEV void wave_compact_topk(ipkey_t* buf, int m, int k, ipkey_t* thr, int* cnt) {
  const int lane = threadIdx.x & 63;
  m = min(m, kScanRoom);
  ipkey_t own[kOwn];
  int rank[kOwn];
#pragma unroll
  for (int r = 0; r < kOwn; ++r) {
    own[r] = r * 64 + lane < m ? buf[r * 64 + lane] : 0;   // 0: no key (a real key is never 0)
    rank[r] = 0;
  }
#pragma unroll
  for (int r = 0; r < kOwn; ++r) {
    const int held = min(64, m - r * 64);
    for (int l = 0; l < held; ++l) {
      const unsigned lo = __builtin_amdgcn_readlane((unsigned)own[r], l);
      const unsigned hi = __builtin_amdgcn_readlane((unsigned)(own[r] >> 32), l);
      const ipkey_t other = ((ipkey_t)hi << 32) | lo;
#pragma unroll
      for (int j = 0; j < kOwn; ++j) rank[j] += other > own[j];
    }
  }
#pragma unroll
  for (int r = 0; r < kOwn; ++r)
    if (own[r] != 0 && rank[r] < k) {
      buf[rank[r]] = own[r];
      if (rank[r] == k - 1) *thr = own[r];
    }
  if (lane == 0) *cnt = min(m, k);
}

// grid.x workgroups; workgroup w takes slabs w, w + grid.x, ...  ws: [grid.x][nq][cap] keys.
template <bool BF16, int QT>
__global__ __launch_bounds__(kThreads) void vcap_ip_scan_kernel(const void* __restrict__ db, long n, int dim,
                                                                const float* __restrict__ queries, int nq, int k,
                                                                ipkey_t* __restrict__ ws, int cap) {
  constexpr int E = BF16 ? 8 : 4;   // elements per 16-byte fragment
  constexpr int H = BF16 ? 2 : 1;   // f32 fragments per load
  constexpr int U = 16 / E;         // steps per 64 elements of a row
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int nsteps = dim / (4 * E);
  u32x4* qimg = reinterpret_cast<u32x4*>(lds_raw);                       // [QT][nsteps][H][64]
  ipkey_t* thr = reinterpret_cast<ipkey_t*>(qimg + QT * nsteps * H * 64);   // [QT * 16]
  int* cnt = reinterpret_cast<int*>(thr + QT * 16);                      // [QT * 16]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;

  for (int i = tid; i < QT * nsteps * H * 64; i += kThreads) {
    const int l = i & 63, h = (i >> 6) % H, s = (i / (64 * H)) % nsteps, t = i / (64 * H * nsteps);
    const int qrow = t * 16 + (l & 15);
    u32x4 v = {0u, 0u, 0u, 0u};
    if (qrow < nq) v = *reinterpret_cast<const u32x4*>(queries + (long)qrow * dim + (s * 4 + (l >> 4)) * E + 4 * h);
    qimg[i] = v;
  }
  if (tid < QT * 16) {
    thr[tid] = 0;
    cnt[tid] = 0;
  }
  __syncthreads();

  ipkey_t* mine = ws + (long)blockIdx.x * nq * cap;
  const size_t row_bytes = (size_t)dim * (BF16 ? 2 : 4);
  const long nslabs = (n + kSlab - 1) / kSlab;
  for (long slab = blockIdx.x; slab < nslabs; slab += gridDim.x) {
    const long row0 = slab * kSlab + (long)wave * (kWaveTiles * 16);
    const unsigned char* rp[kWaveTiles];
#pragma unroll
    for (int rt = 0; rt < kWaveTiles; ++rt)   // rows past the end read the last row; their scores are dropped
      rp[rt] = (const unsigned char*)db + (size_t)min(row0 + rt * 16 + c, n - 1) * row_bytes;
    f32x4 acc[kWaveTiles][QT];
#pragma unroll
    for (int rt = 0; rt < kWaveTiles; ++rt)
#pragma unroll
      for (int t = 0; t < QT; ++t) acc[rt][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // 64 elements of every row per group (U steps); the next group's loads are issued before this
    // group's MFMAs, so a wave keeps 2 * kWaveTiles * U KiB in flight
    u32x4 cur[kWaveTiles][U], nxt[kWaveTiles][U];
#pragma unroll
    for (int rt = 0; rt < kWaveTiles; ++rt)
#pragma unroll
      for (int u = 0; u < U; ++u) cur[rt][u] = *reinterpret_cast<const u32x4*>(rp[rt] + (u * 4 + g) * 16);
    for (int s0 = 0; s0 < nsteps; s0 += U) {
      if (s0 + U < nsteps) {
#pragma unroll
        for (int rt = 0; rt < kWaveTiles; ++rt)
#pragma unroll
          for (int u = 0; u < U; ++u)
            nxt[rt][u] = *reinterpret_cast<const u32x4*>(rp[rt] + ((s0 + U + u) * 4 + g) * 16);
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int t = 0; t < QT; ++t) {
          const u32x4* b = qimg + ((t * nsteps + s0 + u) * H) * 64 + lane;
#pragma unroll
          for (int rt = 0; rt < kWaveTiles; ++rt) {
            if (BF16) {
              acc[rt][t] = mfma_frag(widen_lo(cur[rt][u]), b[0], acc[rt][t], (float*)nullptr);
              acc[rt][t] = mfma_frag(widen_hi(cur[rt][u]), b[64], acc[rt][t], (float*)nullptr);
            } else {
              acc[rt][t] = mfma_frag(cur[rt][u], b[0], acc[rt][t], (float*)nullptr);
            }
          }
        }
#pragma unroll
      for (int rt = 0; rt < kWaveTiles; ++rt)
#pragma unroll
        for (int u = 0; u < U; ++u) cur[rt][u] = nxt[rt][u];
    }
    // accumulator register r of lane (c, g): row 4 g + r of the tile, query c of the query tile
#pragma unroll
    for (int rt = 0; rt < kWaveTiles; ++rt)
#pragma unroll
      for (int t = 0; t < QT; ++t) {
        const int q = t * 16 + c;
        const ipkey_t th = thr[q];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long row = row0 + rt * 16 + 4 * g + r;
          const float sc = acc[rt][t][r];
          if (q < nq && row < n && sc == sc) {
            const ipkey_t key = make_key(sc, (unsigned)row);
            if (key > th) {
              const int pos = atomicAdd(&cnt[q], 1);
              if (pos < cap) mine[(long)q * cap + pos] = key;   // always true: see the compaction rule below
            }
          }
        }
      }
    // Every wave's appends of this slab are in before any counter is read (the barrier comes first: a
    // counter read before it can miss a slower wave's appends, skip a due compaction and let the next
    // slab overrun the buffer).  A buffer that could not take one more slab's keys is compacted now, the
    // queries dealt over the waves.
    __syncthreads();
    for (int q = wave; q < nq; q += kThreads / 64) {
      const int m = __builtin_amdgcn_readfirstlane(cnt[q]);
      if (m > cap - kSlab) wave_compact_topk(mine + (long)q * cap, m, k, &thr[q], &cnt[q]);
    }
    __syncthreads();   // thresholds and counters settled before the next slab's appends
  }
  // leave [q][0, k): the workgroup's best in order, then empty slots
  for (int q = wave; q < nq; q += kThreads / 64) {
    const int m = __builtin_amdgcn_readfirstlane(cnt[q]);
    wave_compact_topk(mine + (long)q * cap, m, k, &thr[q], &cnt[q]);
    for (int j = min(m, k) + lane; j < k; j += 64) mine[(long)q * cap + j] = 0;
  }
}

// One workgroup per query: the k best of the `lists` sorted lists ws[list][query][0, k) -> the outputs.
__global__ __launch_bounds__(kThreads) void vcap_ip_merge_kernel(const ipkey_t* __restrict__ ws, int lists, int nq,
                                                                 int cap, int k, float* __restrict__ out_scores,
                                                                 long long* __restrict__ out_ids) {
  __shared__ ipkey_t buf[kMergeCap];
  __shared__ ipkey_t sel[kMergeCap];
  __shared__ ipkey_t thr;
  __shared__ int cnt;
  const int tid = threadIdx.x, q = blockIdx.x;
  if (tid == 0) {
    thr = 0;
    cnt = 0;
  }
  __syncthreads();
  const long total = (long)lists * k;
  for (long e0 = 0; e0 < total; e0 += kThreads * kMergeLoads) {
    ipkey_t key[kMergeLoads];
#pragma unroll
    for (int u = 0; u < kMergeLoads; ++u) {
      const long e = e0 + u * kThreads + tid;
      key[u] = e < total ? ws[((e / k) * nq + q) * cap + e % k] : 0;
    }
#pragma unroll
    for (int u = 0; u < kMergeLoads; ++u) {
      if (key[u] > thr) {                     // thr >= 0 drops the empty slots
        const int pos = atomicAdd(&cnt, 1);
        if (pos < kMergeCap) buf[pos] = key[u];
      }
      __syncthreads();
      if (cnt > kMergeCap - kThreads) compact_topk(buf, sel, cnt, kMergeCap, k, &thr, &cnt);
      __syncthreads();
    }
  }
  const int m = cnt;
  compact_topk(buf, sel, m, kMergeCap, k, &thr, &cnt);
  for (int j = tid; j < k; j += kThreads) {
    const bool have = j < min(m, k);
    out_scores[(long)q * k + j] = have ? key_score(buf[j]) : -__builtin_inff();
    out_ids[(long)q * k + j] = have ? key_id(buf[j]) : -1;
  }
}

// one wave per row: lane l sums x[l], x[l + 64], ... as one fma chain, then the wave's fixed tree
__global__ __launch_bounds__(kThreads) void vcap_l2_normalize_kernel(const float* x, long ldx, float* y, long ldy,
                                                                     int rows, int dim, float eps, int eps_mode) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * ldx;
  float* yr = y + row * ldy;
  float ss = 0.f;
  for (int i = lane; i < dim; i += 64) ss = fmaf(xr[i], xr[i], ss);
  const float norm = sqrtf(wave_sum(ss));
  const float den = eps_mode ? norm + eps : fmaxf(norm, eps);
  for (int i = lane; i < dim; i += 64) yr[i] = xr[i] / den;
}

// torch's float -> bfloat16: round to nearest even, NaN -> 0x7FC0
VCAP_DEV bf16_t f2bf_torch(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (bf16_t)0x7FC0;
  return (bf16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

template <bool BF16>
__global__ __launch_bounds__(kThreads) void vcap_ip_convert_kernel(const float* __restrict__ x, long ldx, long rows,
                                                                   int dim, void* __restrict__ dst) {
  const long quads = rows * (dim / 4);
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < quads; i += (long)gridDim.x * kThreads) {
    const long r = i / (dim / 4);
    const int col = (int)(i % (dim / 4)) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + r * ldx + col);
    if (BF16) {
      u32x2 o;
      o.x = (uint32_t)f2bf_torch(v.x) | ((uint32_t)f2bf_torch(v.y) << 16);
      o.y = (uint32_t)f2bf_torch(v.z) | ((uint32_t)f2bf_torch(v.w) << 16);
      *reinterpret_cast<u32x2*>((bf16_t*)dst + r * dim + col) = o;
    } else {
      *reinterpret_cast<f32x4*>((float*)dst + r * dim + col) = v;
    }
  }
}

template <bool BF16, int QT>
hipError_t launch_scan(int grid, const void* db, long n, int dim, const float* q, int nq, int k, ipkey_t* ws, int cap,
                       hipStream_t s) {
  const size_t lds = (size_t)QT * 16 * dim * 4 + (size_t)QT * 16 * 12;
  static size_t allowed = 0;   // the largest dynamic LDS size this kernel has been cleared for
  if (lds > allowed) {
    hipError_t e = hipFuncSetAttribute((const void*)vcap_ip_scan_kernel<BF16, QT>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    allowed = lds;
  }
  hipLaunchKernelGGL((vcap_ip_scan_kernel<BF16, QT>), dim3(grid), dim3(kThreads), lds, s, db, n, dim, q, nq, k, ws, cap);
  return hipGetLastError();
}

}  // namespace

int vcap_ip_search_cap(int k) { return k + 2 * kSlab; }

int vcap_ip_search_grid(long n, int max_blocks) {
  const long slabs = (n + kSlab - 1) / kSlab;
  long g = std::min<long>(kIpMaxWorkgroups, 2L * vcap_device_cus());
  if (max_blocks > 0) g = std::min<long>(g, max_blocks);
  return (int)std::max<long>(1, std::min(g, slabs));
}

// query tiles one scan launch holds in LDS at this dim (a power of two: the kernel's instantiations)
int vcap_ip_search_pass_tiles(int dim) {
  const int fit = kIpMaxQueryFloats / (16 * dim);
  return fit >= 4 ? 4 : fit >= 2 ? 2 : 1;
}

hipError_t vcap_ip_search_dispatch(int dt, const void* db, long n, int dim, const float* queries, int nq, int k,
                                   float* out_scores, long long* out_ids, void* workspace, int max_blocks,
                                   hipStream_t s) {
  const int cap = vcap_ip_search_cap(k);
  const int grid = vcap_ip_search_grid(n, max_blocks);
  const int per_pass = vcap_ip_search_pass_tiles(dim) * 16;
  ipkey_t* ws = (ipkey_t*)workspace;
  const bool bf = dt == VCAP_DT_BF16;
  for (int q0 = 0; q0 < nq; q0 += per_pass) {
    const int pq = std::min(per_pass, nq - q0);
    const float* qp = queries + (long)q0 * dim;
    const int qt = pq > 32 ? 4 : pq > 16 ? 2 : 1;
    hipError_t e = hipSuccess;
    if (n > 0) {
      if (bf)
        e = qt == 4   ? launch_scan<true, 4>(grid, db, n, dim, qp, pq, k, ws, cap, s)
            : qt == 2 ? launch_scan<true, 2>(grid, db, n, dim, qp, pq, k, ws, cap, s)
                      : launch_scan<true, 1>(grid, db, n, dim, qp, pq, k, ws, cap, s);
      else
        e = qt == 4   ? launch_scan<false, 4>(grid, db, n, dim, qp, pq, k, ws, cap, s)
            : qt == 2 ? launch_scan<false, 2>(grid, db, n, dim, qp, pq, k, ws, cap, s)
                      : launch_scan<false, 1>(grid, db, n, dim, qp, pq, k, ws, cap, s);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(vcap_ip_merge_kernel, dim3(pq), dim3(kThreads), 0, s, ws, n > 0 ? grid : 0, pq, cap, k,
                       out_scores + (long)q0 * k, out_ids + (long)q0 * k);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// the merge kernel alone, over `lists` sorted lists ws[list][query][0, k) of row stride cap (the IVF list scan's)
hipError_t vcap_ip_merge_dispatch(const void* ws, int lists, int nq, int cap, int k, float* out_scores,
                                  long long* out_ids, hipStream_t s) {
  hipLaunchKernelGGL(vcap_ip_merge_kernel, dim3(nq), dim3(kThreads), 0, s, (const ipkey_t*)ws, lists, nq, cap, k,
                     out_scores, out_ids);
  return hipGetLastError();
}

hipError_t vcap_l2_normalize_dispatch(const float* x, long ldx, float* y, long ldy, int rows, int dim, float eps,
                                      int eps_mode, hipStream_t s) {
  if (rows == 0) return hipSuccess;
  const int per = kThreads / 64;
  hipLaunchKernelGGL(vcap_l2_normalize_kernel, dim3((rows + per - 1) / per), dim3(kThreads), 0, s, x, ldx, y, ldy, rows,
                     dim, eps, eps_mode);
  return hipGetLastError();
}

hipError_t vcap_ip_convert_dispatch(int dt, const float* x, long ldx, long rows, int dim, void* dst, hipStream_t s) {
  if (rows == 0) return hipSuccess;
  const long quads = rows * (dim / 4);
  const int grid = (int)std::min<long>((quads + kThreads - 1) / kThreads, 8L * vcap_device_cus());
  if (dt == VCAP_DT_BF16)
    hipLaunchKernelGGL(vcap_ip_convert_kernel<true>, dim3(grid), dim3(kThreads), 0, s, x, ldx, rows, dim, dst);
  else
    hipLaunchKernelGGL(vcap_ip_convert_kernel<false>, dim3(grid), dim3(kThreads), 0, s, x, ldx, rows, dim, dst);
  return hipGetLastError();
}
