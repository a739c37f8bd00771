// IVF-Flat inner-product index kernels: the coarse assignment of rows to centroids, the spherical k-means
// centroid update, and the scan of the probed inverted lists.  The coarse search over the centroids and the
// final merge are the flat search's own (retrieval.hip).
//
// Scores.  Every inner product here is the flat scan's: a 16-row tile of the stored side (centroids in the
// assignment, list rows in the scan) is the A operand and the query side the B operand of the f32-input
// MFMA, lane (row l & 15, group g = l >> 4) feeding elements [(4 s + g) E, +E) at step s (retrieval.hip's
// header).  A column of the MFMA does not depend on the other columns, so the score of (row, query) has the
// bits vcap_ip_search gives that pair, wherever the row sits in its list and whichever queries share the
// tile.
//
// Assignment.  A workgroup stages up to 64 rows as the query image (read once) and walks the centroid tiles;
// every lane keeps the best key (score, centroid id) of the accumulator cells it owns, and the keys' total
// order (retrieval_common.h) makes the winner the largest score, lowest id on ties; a NaN score makes no key.
//
// List scan.  Work item (query, probe, slice): the workgroup scores one slice (kIvfSliceRows rows) of the
// probed list against its one query - the query fills all 16 MFMA columns, column 0 is read - collects the
// slice's keys (score, original id) in LDS, ranks them by counting and leaves its best k, in order, in the
// workspace: a function of the key set alone.  Rows of a tile past the slice's end read the slice's last row
// and are dropped (list starts are not padded).  Items past their list's end leave k empty slots.
//
// Centroid update.  Slot t = offsets[l] / chunk + l + c holds the sum of chunk c of list l (the map is
// injective and bounded by n / chunk + nlist + 1 without knowing any list's length on the host); one wave
// sums a chunk's rows in `order` order, a second kernel adds a list's partials in chunk order and
// normalises with vcap_l2_normalize's mode-0 arithmetic.  No atomics: a centroid is a function of its
// member rows in order.
#include "retrieval_common.h"
#include "vcap_common.h"
#include "vcap_kernels.h"

#include <algorithm>

namespace {

constexpr int kThreads = kIpThreads;
constexpr int kWaves = kThreads / 64;
constexpr int kWaveTiles = 2;                          // 16-row tiles per wave and slab, as the flat scan
constexpr int kSlab = kWaves * kWaveTiles * 16;        // stored rows per workgroup step
static_assert(kIvfSliceRows % kSlab == 0, "a slice is whole slabs");

VCAP_DEV ipkey_t key_max(ipkey_t a, ipkey_t b) { return a > b ? a : b; }
VCAP_DEV ipkey_t key_shfl_xor(ipkey_t v, int mask) {
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, mask);
  const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), mask);
  return ((ipkey_t)hi << 32) | lo;
}

// ---------------------------------------------------------------------------------------------- assignment
// workgroup b takes rows [b * QT * 16, +QT * 16) of x and every centroid
template <int QT>
__global__ __launch_bounds__(kThreads) void vcap_ivf_assign_kernel(const float* __restrict__ x, long ldx, long n,
                                                                   const float* __restrict__ cent, int nlist, int dim,
                                                                   int* __restrict__ assign,
                                                                   float* __restrict__ score) {
  constexpr int U = 4;   // steps per 64 elements of a row (f32: 4 elements per 16-byte fragment)
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int nsteps = dim / 16;
  u32x4* qimg = reinterpret_cast<u32x4*>(lds_raw);                         // [QT][nsteps][64]
  ipkey_t* wbest = reinterpret_cast<ipkey_t*>(qimg + QT * nsteps * 64);    // [kWaves][QT * 16]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const long r0 = (long)blockIdx.x * (QT * 16);

  for (int i = tid; i < QT * nsteps * 64; i += kThreads) {
    const int l = i & 63, s = (i >> 6) % nsteps, t = i / (64 * nsteps);
    const long qrow = r0 + t * 16 + (l & 15);
    u32x4 v = {0u, 0u, 0u, 0u};
    if (qrow < n) v = *reinterpret_cast<const u32x4*>(x + qrow * ldx + (s * 4 + (l >> 4)) * 4);
    qimg[i] = v;
  }
  __syncthreads();

  ipkey_t best[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) best[t] = 0;
  const size_t row_bytes = (size_t)dim * 4;
  const int nslabs = (nlist + kSlab - 1) / kSlab;
  for (int slab = 0; slab < nslabs; ++slab) {
    const int row0 = slab * kSlab + wave * (kWaveTiles * 16);
    const unsigned char* rp[kWaveTiles];
#pragma unroll
    for (int rt = 0; rt < kWaveTiles; ++rt)   // centroids past the end read the last one; their scores are dropped
      rp[rt] = (const unsigned char*)cent + (size_t)min(row0 + rt * 16 + c, nlist - 1) * row_bytes;
    f32x4 acc[kWaveTiles][QT];
#pragma unroll
    for (int rt = 0; rt < kWaveTiles; ++rt)
#pragma unroll
      for (int t = 0; t < QT; ++t) acc[rt][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
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
          const u32x4 b = qimg[(t * nsteps + s0 + u) * 64 + lane];
#pragma unroll
          for (int rt = 0; rt < kWaveTiles; ++rt) acc[rt][t] = mfma_frag(cur[rt][u], b, acc[rt][t], (float*)nullptr);
        }
#pragma unroll
      for (int rt = 0; rt < kWaveTiles; ++rt)
#pragma unroll
        for (int u = 0; u < U; ++u) cur[rt][u] = nxt[rt][u];
    }
    // accumulator register r of lane (c, g): centroid 4 g + r of the tile, row c of the row tile
#pragma unroll
    for (int rt = 0; rt < kWaveTiles; ++rt)
#pragma unroll
      for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int cid = row0 + rt * 16 + 4 * g + r;
          const float sc = acc[rt][t][r];
          if (cid < nlist && sc == sc) best[t] = key_max(best[t], make_key(sc, (unsigned)cid));
        }
  }
  // the four lane groups of a wave, then the waves
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    best[t] = key_max(best[t], key_shfl_xor(best[t], 16));
    best[t] = key_max(best[t], key_shfl_xor(best[t], 32));
    if (g == 0) wbest[wave * (QT * 16) + t * 16 + c] = best[t];
  }
  __syncthreads();
  if (tid < QT * 16) {
    ipkey_t b = wbest[tid];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) b = key_max(b, wbest[w * (QT * 16) + tid]);
    const long row = r0 + tid;
    if (row < n) {
      assign[row] = b ? (int)key_id(b) : -1;
      if (score) score[row] = b ? key_score(b) : -__builtin_inff();
    }
  }
}

template <int QT>
hipError_t launch_assign(const float* x, long ldx, long n, const float* cent, int nlist, int dim, int* assign,
                         float* score, hipStream_t s) {
  const size_t lds = (size_t)QT * 16 * dim * 4 + (size_t)kWaves * QT * 16 * sizeof(ipkey_t);
  static size_t allowed = 0;   // the largest dynamic LDS size this kernel has been cleared for
  if (lds > allowed) {
    hipError_t e = hipFuncSetAttribute((const void*)vcap_ivf_assign_kernel<QT>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    allowed = lds;
  }
  const long grid = (n + QT * 16 - 1) / (QT * 16);
  hipLaunchKernelGGL((vcap_ivf_assign_kernel<QT>), dim3((unsigned)grid), dim3(kThreads), lds, s, x, ldx, n, cent, nlist,
                     dim, assign, score);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- list scan
// grid (slices, nprobe, nq).  keys: [probe * slices + slice][query][k]
template <bool BF16>
__global__ __launch_bounds__(kThreads) void vcap_ivf_scan_kernel(const void* __restrict__ rows,
                                                                 const long long* __restrict__ ids,
                                                                 const long long* __restrict__ offsets, long ntotal,
                                                                 int nlist, int dim, const float* __restrict__ queries,
                                                                 int nq, const long long* __restrict__ probes,
                                                                 int nprobe, int k, ipkey_t* __restrict__ keys) {
  constexpr int E = BF16 ? 8 : 4;   // elements per 16-byte fragment
  constexpr int U = 16 / E;         // steps per 64 elements of a row
  __shared__ __attribute__((aligned(16))) float qv[1024];
  __shared__ ipkey_t buf[kIvfSliceRows];
  __shared__ ipkey_t sel[kIvfSliceRows];
  __shared__ ipkey_t thr;
  __shared__ int cnt;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int slice = blockIdx.x, p = blockIdx.y, q = blockIdx.z;
  ipkey_t* out = keys + (((long)p * gridDim.x + slice) * nq + q) * k;

  // the slice's rows [beg, end) of the grouped table; nothing to do for a filler probe, a slice past the
  // list's end, or offsets that do not lie in [0, ntotal]
  const long long list = probes[(long)q * nprobe + p];
  long beg = 0, end = 0;
  if (list >= 0 && list < nlist) {
    const long lb = (long)offsets[list], le = (long)offsets[list + 1];
    if (lb >= 0 && le <= ntotal) {
      beg = lb + (long)slice * kIvfSliceRows;
      end = min(le, beg + (long)kIvfSliceRows);
    }
  }
  if (beg >= end) {   // workgroup-uniform
    for (int j = tid; j < k; j += kThreads) out[j] = 0;
    return;
  }

  for (int i = tid; i < dim; i += kThreads) qv[i] = queries[(long)q * dim + i];
  if (tid == 0) {
    thr = 0;
    cnt = 0;
  }
  __syncthreads();

  const int nsteps = dim / (4 * E);
  const size_t row_bytes = (size_t)dim * (BF16 ? 2 : 4);
  for (long slab0 = beg; slab0 < end; slab0 += kSlab) {
    const long row0 = slab0 + (long)wave * (kWaveTiles * 16);
    const unsigned char* rp[kWaveTiles];
#pragma unroll
    for (int rt = 0; rt < kWaveTiles; ++rt)   // rows past the slice's end read its last row; their scores are dropped
      rp[rt] = (const unsigned char*)rows + (size_t)min(row0 + rt * 16 + c, end - 1) * row_bytes;
    f32x4 acc[kWaveTiles];
#pragma unroll
    for (int rt = 0; rt < kWaveTiles; ++rt) acc[rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
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
      for (int u = 0; u < U; ++u) {
        // the query's elements [(4 s + g) E, +E): the same in all 16 columns
        const u32x4* b = reinterpret_cast<const u32x4*>(qv + ((s0 + u) * 4 + g) * E);
#pragma unroll
        for (int rt = 0; rt < kWaveTiles; ++rt) {
          if (BF16) {
            acc[rt] = mfma_frag(widen_lo(cur[rt][u]), b[0], acc[rt], (float*)nullptr);
            acc[rt] = mfma_frag(widen_hi(cur[rt][u]), b[1], acc[rt], (float*)nullptr);
          } else {
            acc[rt] = mfma_frag(cur[rt][u], b[0], acc[rt], (float*)nullptr);
          }
        }
      }
#pragma unroll
      for (int rt = 0; rt < kWaveTiles; ++rt)
#pragma unroll
        for (int u = 0; u < U; ++u) cur[rt][u] = nxt[rt][u];
    }
    // accumulator register r of lane (c, g): row 4 g + r of the tile; column 0 speaks for the query
    if (c == 0) {
#pragma unroll
      for (int rt = 0; rt < kWaveTiles; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long row = row0 + rt * 16 + 4 * g + r;
          const float sc = acc[rt][r];
          if (row < end && sc == sc) {
            const int pos = atomicAdd(&cnt, 1);
            if (pos < kIvfSliceRows) buf[pos] = make_key(sc, (unsigned)ids[row]);   // always true: one key per row
          }
        }
    }
  }
  __syncthreads();
  const int m = min(cnt, kIvfSliceRows);
  compact_topk(buf, sel, m, kIvfSliceRows, k, &thr, &cnt);
  for (int j = tid; j < k; j += kThreads) out[j] = j < min(m, k) ? buf[j] : 0;
}

// ---------------------------------------------------------------------------------------------- centroid update
VCAP_DEV long slot0_of(const long long* offsets, int l) { return (long)(offsets[l] / kIvfChunkRows) + l; }

// one wave per slot: lane l sums elements [4 l + 256 j, +4) of the chunk's rows, in `order` order
__global__ __launch_bounds__(kThreads) void vcap_ivf_partial_kernel(const float* __restrict__ x, long ldx, long n,
                                                                    int dim, const long long* __restrict__ order,
                                                                    const long long* __restrict__ offsets, int nlist,
                                                                    long nslots, float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const long t = (long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (t >= nslots) return;
  int lo = 0, hi = nlist - 1;   // the last list whose first slot is <= t (first slots increase strictly)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (slot0_of(offsets, mid) <= t) lo = mid; else hi = mid - 1;
  }
  const long ch = t - slot0_of(offsets, lo);
  const long lb = (long)offsets[lo], len = (long)offsets[lo + 1] - lb;
  if (ch < 0 || ch * kIvfChunkRows >= len) return;   // a slot no chunk maps to
  const long beg = lb + ch * kIvfChunkRows;
  const int rows = (int)min((long)kIvfChunkRows, len - ch * kIvfChunkRows);
  if (beg < 0 || beg + rows > n) return;             // offsets outside the order array: read nothing
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int col = 4 * lane;
  for (int i0 = 0; i0 < rows; i0 += 4) {
    f32x4 v[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long idx = i0 + i < rows ? order[beg + i0 + i] : -1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (idx >= 0 && idx < n && col + 256 * j < dim) v[i][j] = *reinterpret_cast<const f32x4*>(x + idx * ldx + col + 256 * j);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i0 + i < rows) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += v[i][j];
      }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (col + 256 * j < dim) *reinterpret_cast<f32x4*>(part + t * dim + col + 256 * j) = acc[j];
}

// one wave per list: its partials in chunk order, then vcap_l2_normalize's mode-0 arithmetic (lane l holds
// elements l, l + 64, ...; the sum of squares one fma chain per lane and the wave's fixed tree)
__global__ __launch_bounds__(kThreads) void vcap_ivf_finish_kernel(const float* __restrict__ part, long nslots,
                                                                   const long long* __restrict__ offsets, int nlist,
                                                                   int dim, const float* prev, float* out, float eps) {
  const int lane = threadIdx.x & 63;
  const int l = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (l >= nlist) return;
  const long len = (long)(offsets[l + 1] - offsets[l]);
  const long s0 = slot0_of(offsets, l), nch = (len + kIvfChunkRows - 1) / kIvfChunkRows;
  if (len <= 0 || s0 < 0 || s0 + nch > nslots) {   // an empty list keeps its centroid
    if (out != prev)
      for (int i = lane; i < dim; i += 64) out[(long)l * dim + i] = prev[(long)l * dim + i];
    return;
  }
  float v[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = lane + 64 * j < dim ? part[s0 * dim + lane + 64 * j] : 0.f;
  for (long ch = 1; ch < nch; ++ch) {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (lane + 64 * j < dim) v[j] += part[(s0 + ch) * dim + lane + 64 * j];
  }
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (lane + 64 * j < dim) ss = fmaf(v[j], v[j], ss);
  const float norm = sqrtf(wave_sum(ss));
  const float den = fmaxf(norm, eps);
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (lane + 64 * j < dim) out[(long)l * dim + lane + 64 * j] = v[j] / den;
}

}  // namespace

hipError_t vcap_ivf_assign_dispatch(const float* x, long ldx, long n, const float* centroids, int nlist, int dim,
                                    int* assign, float* score, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const int fit = vcap_ip_search_pass_tiles(dim);   // row tiles whose image fits LDS at this dim
  const int qt = std::min<long>(fit, n > 32 ? 4 : n > 16 ? 2 : 1);
  return qt == 4   ? launch_assign<4>(x, ldx, n, centroids, nlist, dim, assign, score, s)
         : qt == 2 ? launch_assign<2>(x, ldx, n, centroids, nlist, dim, assign, score, s)
                   : launch_assign<1>(x, ldx, n, centroids, nlist, dim, assign, score, s);
}

long vcap_ivf_update_slots(long n, int nlist) { return n / kIvfChunkRows + nlist + 1; }

hipError_t vcap_ivf_centroid_update_dispatch(const float* x, long ldx, long n, int dim, const long long* order,
                                             const long long* offsets, int nlist, const float* prev, float* out,
                                             float eps, float* partials, hipStream_t s) {
  const long nslots = vcap_ivf_update_slots(n, nlist);
  hipLaunchKernelGGL(vcap_ivf_partial_kernel, dim3((unsigned)((nslots + kWaves - 1) / kWaves)), dim3(kThreads), 0, s, x,
                     ldx, n, dim, order, offsets, nlist, nslots, partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(vcap_ivf_finish_kernel, dim3((unsigned)((nlist + kWaves - 1) / kWaves)), dim3(kThreads), 0, s,
                     partials, nslots, offsets, nlist, dim, prev, out, eps);
  return hipGetLastError();
}

hipError_t vcap_ivf_search_dispatch(int dt, const void* rows, const long long* ids, const long long* offsets, long ntotal,
                                    const float* centroids, int nlist, long max_list_len, int dim,
                                    const float* queries, int nq, int nprobe, int k, float* out_scores,
                                    long long* out_ids, long long* probes, float* probe_scores, void* coarse_ws,
                                    void* keys, int max_blocks, hipStream_t s) {
  // (a) the nprobe best centroids per query: the flat search over the centroid table
  hipError_t e = vcap_ip_search_dispatch(VCAP_DT_F32, centroids, nlist, dim, queries, nq, nprobe, probe_scores, probes,
                                         coarse_ws, max_blocks, s);
  if (e != hipSuccess) return e;
  // (b) one workgroup per (query, probe, slice)
  const int slices = (int)((max_list_len + kIvfSliceRows - 1) / kIvfSliceRows);
  if (slices > 0) {
    const dim3 grid((unsigned)slices, (unsigned)nprobe, (unsigned)nq);
    if (dt == VCAP_DT_BF16)
      hipLaunchKernelGGL(vcap_ivf_scan_kernel<true>, grid, dim3(kThreads), 0, s, rows, ids, offsets, ntotal, nlist, dim,
                         queries, nq, probes, nprobe, k, (ipkey_t*)keys);
    else
      hipLaunchKernelGGL(vcap_ivf_scan_kernel<false>, grid, dim3(kThreads), 0, s, rows, ids, offsets, ntotal, nlist, dim,
                         queries, nq, probes, nprobe, k, (ipkey_t*)keys);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  // (c) the k best of every item's list, per query
  return vcap_ip_merge_dispatch(keys, nprobe * slices, nq, k, k, out_scores, out_ids, s);
}
