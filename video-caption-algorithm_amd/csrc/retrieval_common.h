// Device helpers shared by the retrieval kernels (retrieval.hip: the flat scan and merge; ivf.hip: the
// coarse assignment and the list scan): the 64-bit (score, id) key and its total order, the workgroup's
// exact top-k selection by counting, and the bf16 -> f32 widening of a 16-byte fragment.
#pragma once
#include "vcap_common.h"

typedef unsigned long long ipkey_t;

constexpr int kIpThreads = 256;   // threads of every retrieval workgroup (compact_topk strides by it)

// The score's bits mapped monotonically to an unsigned integer in the high word, 0xFFFFFFFF - id in the
// low word: key_a > key_b <=> (score_a > score_b) or (equal scores and id_a < id_b).  0 is the empty slot
// (a real key's low word is >= 2^31).
VCAP_DEV ipkey_t make_key(float score, unsigned id) {
  unsigned b = __float_as_uint(score + 0.0f);                  // -0 -> +0: equal scores, equal bits
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((ipkey_t)b << 32) | (ipkey_t)(0xFFFFFFFFu - id);
}
VCAP_DEV float key_score(ipkey_t k) {
  const unsigned b = (unsigned)(k >> 32);
  return __uint_as_float((b & 0x80000000u) ? (b & 0x7FFFFFFFu) : ~b);
}
VCAP_DEV long long key_id(ipkey_t k) { return (long long)(0xFFFFFFFFu - (unsigned)k); }

// The m keys of buf -> their best min(m, k) in descending order in buf[0 ..), *thr = the k-th best where
// there are k, *cnt = min(m, k).  Every thread of the workgroup calls it with the same arguments, after a
// barrier that follows the last append; sel is LDS scratch of `room` keys (m never exceeds it by the
// callers' append rule; the clamp keeps a broken rule from becoming an out-of-bounds access).  Ends with a
// barrier.
VCAP_DEV void compact_topk(ipkey_t* buf, ipkey_t* sel, int m, int room, int k, ipkey_t* thr, int* cnt) {
  m = min(m, room);
  for (int i = threadIdx.x; i < m; i += kIpThreads) sel[i] = buf[i];
  __syncthreads();
  for (int i = threadIdx.x; i < m; i += kIpThreads) {
    const ipkey_t key = sel[i];
    int rank = 0;
    for (int j = 0; j < m; ++j) rank += sel[j] > key;
    if (rank < k) buf[rank] = key;
    if (rank == k - 1) *thr = key;
  }
  if (threadIdx.x == 0) *cnt = min(m, k);
  __syncthreads();
}

// the two f32 fragments of a 16-byte load of 8 bf16 (element 2 i in the low half of dword i)
VCAP_DEV u32x4 widen_lo(u32x4 v) { return (u32x4){v.x << 16, v.x & 0xFFFF0000u, v.y << 16, v.y & 0xFFFF0000u}; }
VCAP_DEV u32x4 widen_hi(u32x4 v) { return (u32x4){v.z << 16, v.z & 0xFFFF0000u, v.w << 16, v.w & 0xFFFF0000u}; }
