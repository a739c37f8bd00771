// The decoder's single-query causal attention over the paged K/V pools: one wave per (row m, head h)
// item, positions 0..past+i of the row's sequence.  Two kernel templates - any context up to 1024,
// and contexts of at most 64 with every load of the item issued at once - each templated on where a
// key's page comes from (the key-source policies below), so greedy decode, teacher-forced scoring and
// beam search run ONE copy of the arithmetic:
//   scores: lane <-> key, dims 0..63 summed in order, then * 0.125;  p = the fast exp of (s - max);  the row sum is
//   a wave sum of per-lane sums;  P.V: lane = (key group kg of 8, 8 consecutive dims d8), keys kg,
//   kg + 8, ... in order (clamped rows add 0 * v), the 8 groups reduced by DPP + permlane swaps
//   (rows_sum(o + dpp_f<0x128>(o)));  the scale by 1 / sum at the store.
// Pool layout: element d of position j of a sequence, head h = pool[((page * H + h) * 16 + (j & 15)) * 64 + d].
#include "vcap_common.h"
#include "vcap_kernels.h"

// ------------------------------------------------------------------------------------------------
// Key sources.  A policy is a kernel argument; item() / item64() set up what one (row, head) item of
// the general / the <= 64 kernel needs (seq = the row's sequence, m = the row), and the item answers
//   page(j)           the page that holds key j (any j < ctx, any lane)
//   own_page(jk)      the same for jk = min(lane, ctx - 1), the key this lane scores in the <= 64 kernel
// kSingleQuery: every row is a sequence of its own (S_new == 1, seq == m).  kStaged: item64 reads memory
// and writes this wave's 64 ints of LDS (s_a), so the <= 64 kernel has a first round trip: c64_issue puts
// the query into it too and owns the wave barrier that publishes both.  kPvUnroll: the unroll count the
// general kernel asks for on its P.V loop (0: none), the parent kernels' own, kept per path
// (profiles/decode_attention_refactor_resources.txt).

// Page table [seqs][maxp] (maxp <= 64): lane p holds page p of the sequence, read once and broadcast,
// so no K/V load waits on a dependent page-table load.
struct PagedKeys {
  static constexpr bool kSingleQuery = false, kStaged = false;
  static constexpr int kPvUnroll = 4;
  const int* table;
  int maxp;
  struct Item {
    int mine;
    VCAP_DEV int page(int j) const { return __shfl(mine, j >> 4); }
    VCAP_DEV int own_page(int jk) const { return page(jk); }
  };
  VCAP_DEV Item item(int seq, int) const { return {table[seq * maxp + min((int)threadIdx.x & 63, maxp - 1)]}; }
  VCAP_DEV Item item64(int seq, int m, int, int*) const { return item(seq, m); }
};

// The contiguous layout the runtime allocates (the identity page table): computed, no load at all.
struct ContiguousKeys {
  static constexpr bool kSingleQuery = false, kStaged = false;
  static constexpr int kPvUnroll = 4;
  int maxp;
  struct Item {
    int first;
    VCAP_DEV int page(int j) const { return first + (j >> 4); }
    VCAP_DEV int own_page(int jk) const { return page(jk); }
  };
  VCAP_DEV Item item(int seq, int) const { return {seq * maxp}; }
  VCAP_DEV Item item64(int seq, int m, int, int*) const { return item(seq, m); }
};

// Beam search's ancestry table: key j of row m is position j of physical row anc[m * anc_ld + j] of the
// contiguous layout (no K/V copies on a reorder).  General form: one dependent load per key.  <= 64
// form: the entry of key `lane` is read first (with the query) and shared through LDS, so the item pays
// two memory round trips (entries and q, then K / V together) instead of two per 8-key group.
struct AncestryKeys {
  static constexpr bool kSingleQuery = true, kStaged = true;
  static constexpr int kPvUnroll = 0;  // the compiler's own choice
  const int* anc;
  int anc_ld, maxp;
  struct Item {
    const int* row;
    int maxp;
    VCAP_DEV int page(int j) const { return row[j] * maxp + (j >> 4); }
  };
  struct Item64 {
    const int* s_a;  // LDS: entry of key min(lane', ctx - 1) for every lane'
    int mine, maxp;
    VCAP_DEV int page(int j) const { return s_a[j] * maxp + (j >> 4); }
    VCAP_DEV int own_page(int jk) const { return mine * maxp + (jk >> 4); }
  };
  VCAP_DEV Item item(int, int m) const { return {anc + (long)m * anc_ld, maxp}; }
  VCAP_DEV Item64 item64(int, int m, int ctx, int* s_a) const {
    const int lane = threadIdx.x & 63;
    const int mine = anc[(long)m * anc_ld + min(lane, ctx - 1)];
    s_a[lane] = mine;
    return {s_a, mine, maxp};
  }
};

// Optional per-sequence key mask (teacher-forced scoring: vcap_gpt2_score).  A hidden key's score is
// -inf before the softmax.  KeyMask<false> is empty and hides nothing, so the unmasked instantiations
// are the kernels every decode step runs.  Key 0 of every sequence must be visible (a row with no
// visible key has no softmax).
template <bool MASKED>
struct KeyMask {
  VCAP_DEV bool hidden(int, int) const { return false; }
};
template <>
struct KeyMask<true> {
  const uint8_t* m;  // [seqs][ld]: 0 = key hidden from every query of its sequence
  int ld;
  VCAP_DEV bool hidden(int seq, int j) const { return m[(long)seq * ld + j] == 0; }
};

// Row positions: which sequence row m belongs to and the position its query sits at (ctx = position + 1).
// UniformRows is (S_new, past): sequence m / S_new, position past + m % S_new - every call with one prompt
// for the batch.  TableRows reads them (ragged prompts): sequence row_seq[m] (nullptr: m), position
// row_pos[m] + pos_add, so rows of one launch stop at contexts of their own; each item still runs the
// same loop to its own ctx, in the same order.
// The two kernel forms do not give the same f32 bits, and a one-prompt call picks its form by the
// sequence's length at the launch (past + S_new <= 64).  A ragged launch keeps every row on the form its
// own one-prompt call takes: mine() passes the rows whose sequence length is in (lo, hi], and a launch
// with sequences on both sides of 64 runs both kernels, each on its own rows.
struct UniformRows {
  int S_new, past;
  VCAP_DEV void locate(int m, bool single, int& seq, int& qpos) const {
    const int S = single ? 1 : S_new;
    seq = m / S;
    qpos = past + (m - seq * S);
  }
  VCAP_DEV bool mine(int, int) const { return true; }
};
struct TableRows {
  const int* row_seq;
  const int* row_pos;
  int pos_add;
  const int* seq_len;  // [seqs] with row_seq (a packed prefill: the sequence's S0); else the row's own ctx
  int lo, hi;
  VCAP_DEV void locate(int m, bool, int& seq, int& qpos) const {
    seq = row_seq ? row_seq[m] : m;
    qpos = row_pos[m] + pos_add;
  }
  VCAP_DEV bool mine(int seq, int ctx) const {
    const int len = row_seq ? seq_len[seq] : ctx;
    return len > lo && len <= hi;
  }
};

// ------------------------------------------------------------------------------------------------
// the E8 elements of a 16-byte chunk as floats, in memory order
template <typename T>
VCAP_DEV void chunk_to_f(const u32x4& v, float (&f)[Frag<T>::kElems]) {
  if constexpr (sizeof(T) == 2) {
    const unsigned w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      f[2 * e] = bf2f((bf16_t)(w4[e] & 0xffff));
      f[2 * e + 1] = bf2f((bf16_t)(w4[e] >> 16));
    }
  } else {
    const f32x4 v4 = __builtin_bit_cast(f32x4, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = v4[e];
  }
}

// 8 consecutive output dims o[] * inv -> orow (16-byte aligned)
template <typename T>
VCAP_DEV void store_out8(T* orow, const float (&o)[8], float inv) {
  if constexpr (sizeof(T) == 2) {
    *reinterpret_cast<u32x4*>(orow) =
        (u32x4){pack_bf2(o[0] * inv, o[1] * inv), pack_bf2(o[2] * inv, o[3] * inv),
                pack_bf2(o[4] * inv, o[5] * inv), pack_bf2(o[6] * inv, o[7] * inv)};
  } else {
    *reinterpret_cast<f32x4*>(orow) = (f32x4){o[0], o[1], o[2], o[3]} * inv;
    *reinterpret_cast<f32x4*>(orow + 4) = (f32x4){o[4], o[5], o[6], o[7]} * inv;
  }
}

// ------------------------------------------------------------------------------------------------
// Any context up to 1024 (the dispatcher's bound: s_p).  4 items per 256-thread workgroup.
// Scores: lane j <-> key j (+64 ...), full 64-dim dot.  P.V: lane = (key group kg of 8, 8
// consecutive dims d8), partial sums reduced over the 8 key groups by DPP + permlane swaps.
template <typename T, typename Keys, bool MASKED, typename Rows = UniformRows>
__global__ __launch_bounds__(256) void vcap_decode_attention_kernel(const T* __restrict__ q, const T* __restrict__ kc,
                                                                    const T* __restrict__ vc, Keys keys,
                                                                    T* __restrict__ out, int M, int H, Rows rows,
                                                                    KeyMask<MASKED> km) {
  constexpr int E8 = Frag<T>::kElems;  // elements per 16-byte chunk
  __shared__ float s_q[4][64];
  __shared__ float s_p[4][1024];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int item = blockIdx.x * 4 + wave;
  if (item >= M * H) return;
  const int m = item / H, h = item - m * H;
  const int E = H * 64;
  int seq, qpos;
  rows.locate(m, Keys::kSingleQuery, seq, qpos);
  const int ctx = qpos + 1;
  if (!rows.mine(seq, ctx)) return;
  const auto ki = keys.item(seq, m);
  s_q[wave][lane] = Num<T>::to_f(q[(long)m * E + h * 64 + lane]);
  __builtin_amdgcn_wave_barrier();
  float mx = -INFINITY;
  for (int j0 = 0; j0 < ctx; j0 += 64) {
    const int j = min(j0 + lane, ctx - 1);
    const T* krow = kc + (((long)ki.page(j) * H + h) * 16 + (j & 15)) * 64;
    u32x4 kv[64 / E8];
#pragma unroll
    for (int c = 0; c < 64 / E8; ++c) kv[c] = *reinterpret_cast<const u32x4*>(krow + c * E8);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 64 / E8; ++c) {
      const T* ke = reinterpret_cast<const T*>(&kv[c]);
#pragma unroll
      for (int e = 0; e < E8; ++e) s += s_q[wave][c * E8 + e] * Num<T>::to_f(ke[e]);
    }
    s *= 0.125f;
    if (j0 + lane < ctx) {
      if constexpr (MASKED)
        if (km.hidden(seq, j0 + lane)) s = -INFINITY;
      s_p[wave][j0 + lane] = s;
      mx = fmaxf(mx, s);
    }
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < ctx; j += 64) {
    const float p = __expf(s_p[wave][j] - mx);
    s_p[wave][j] = p;
    sum += p;
  }
  sum = wave_sum(sum);
  __builtin_amdgcn_wave_barrier();
  const int kg = lane >> 3, d8 = (lane & 7) * 8;
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;
  auto pv_step = [&](int j0) {
    const int jj = j0 + kg;
    const int j = min(jj, ctx - 1);
    const T* vrow = vc + (((long)ki.page(j) * H + h) * 16 + (j & 15)) * 64 + d8;
    const float p = jj < ctx ? s_p[wave][j] : 0.f;
#pragma unroll
    for (int v = 0; v < 8 / E8; ++v) {
      float f[E8];
      chunk_to_f<T>(*reinterpret_cast<const u32x4*>(vrow + v * E8), f);
#pragma unroll
      for (int e = 0; e < E8; ++e) o[v * E8 + e] += p * f[e];
    }
  };
  if constexpr (Keys::kPvUnroll > 0) {
#pragma unroll Keys::kPvUnroll
    for (int j0 = 0; j0 < ctx; j0 += 8) pv_step(j0);
  } else {
    for (int j0 = 0; j0 < ctx; j0 += 8) pv_step(j0);
  }
  // reduce over the 8 key groups: lane ^ 8 (row_ror:8 inside a 16-lane row), then ^16, ^32
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = rows_sum(o[e] + dpp_f<0x128>(o[e]));
  if (kg == 0) store_out8<T>(out + (long)m * E + h * 64 + d8, o, 1.0f / sum);
}

// ------------------------------------------------------------------------------------------------
// Contexts of at most 64, on ONE wave per item: scores with lane = key, P.V with lane = (key group,
// 8 dims) as above.  c64_issue issues every load of the item at once (q, the lane's K row, its 8 V
// rows: one memory round trip); for a kStaged key source the query (one element per lane, straight to
// s_q) rides the source's own first round trip instead, which also keeps the f32 instantiation from
// holding q, K and V in registers together.  c64_finish is the arithmetic, in the general kernel's
// operation order (tests/test_gpu_bf16.py holds the two to the same bits).
template <typename T>
struct C64Loads {
  static constexpr int E8 = Frag<T>::kElems, NK = 64 / E8, NV = 8 / E8;  // bf16: 8, 8, 1; f32: 4, 16, 2
  u32x4 q;          // E8 of the head's 64 query dims: chunk (lane & (NK - 1)); unused when kStaged
  u32x4 kv[NK];     // K row of key min(lane, ctx - 1)
  u32x4 vv[8][NV];  // V rows of keys it * 8 + kg (clamped), dims [d8, d8 + 8)
};

template <typename T, typename Keys>
VCAP_DEV void c64_issue(C64Loads<T>& L, const T* q, const T* kc, const T* vc, const Keys& keys, int seq, int m, int h,
                        int H, int ctx, float* s_q, int* s_a) {
  constexpr int E8 = C64Loads<T>::E8, NK = C64Loads<T>::NK, NV = C64Loads<T>::NV;
  const int lane = threadIdx.x & 63, kg = lane >> 3, d8 = (lane & 7) * 8;
  auto row_of = [&](int page, int j) { return (((long)page * H + h) * 16 + (j & 15)) * 64; };
  auto ld = [](const T* base, long elem) { return *reinterpret_cast<const u32x4*>(base + elem); };
  float qe = 0.f;
  if constexpr (Keys::kStaged) qe = Num<T>::to_f(q[(long)m * H * 64 + h * 64 + lane]);
  else L.q = ld(q, (long)m * H * 64 + h * 64 + (lane & (NK - 1)) * E8);
  const auto ki = keys.item64(seq, m, ctx, s_a);
  if constexpr (Keys::kStaged) {
    s_q[lane] = qe;
    __builtin_amdgcn_wave_barrier();
  }
  const int jk = min(lane, ctx - 1);
  const long kr = row_of(ki.own_page(jk), jk);
#pragma unroll
  for (int c = 0; c < NK; ++c) L.kv[c] = ld(kc, kr + c * E8);
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int j = min(it * 8 + kg, ctx - 1);
    const long vr = row_of(ki.page(j), j) + d8;
#pragma unroll
    for (int v = 0; v < NV; ++v) L.vv[it][v] = ld(vc, vr + v * E8);
  }
}

// s_q / s_p: this wave's 64 floats each of LDS (s_q 16-byte aligned; Q_STAGED: c64_issue has filled it);
// orow = out + m * E + h * 64; vis: key `lane` is not hidden by a key mask
template <typename T, bool Q_STAGED>
VCAP_DEV void c64_finish(const C64Loads<T>& L, float* s_q, float* s_p, int ctx, T* orow, bool vis = true) {
  constexpr int E8 = C64Loads<T>::E8, NK = C64Loads<T>::NK, NV = C64Loads<T>::NV;
  const int lane = threadIdx.x & 63, kg = lane >> 3, d8 = (lane & 7) * 8;
  float f[E8];
  if constexpr (!Q_STAGED) {
    if (lane < NK) {
      chunk_to_f<T>(L.q, f);
#pragma unroll
      for (int e = 0; e < E8; ++e) s_q[lane * E8 + e] = f[e];
    }
    __builtin_amdgcn_wave_barrier();
  }
  float sc = 0.f;
#pragma unroll
  for (int c = 0; c < NK; ++c) {
    chunk_to_f<T>(L.kv[c], f);
#pragma unroll
    for (int e = 0; e < E8; ++e) sc += s_q[c * E8 + e] * f[e];
  }
  sc *= 0.125f;
  const bool live = lane < ctx && vis;
  const float mx = wave_max(live ? sc : -INFINITY);
  const float p = live ? __expf(sc - mx) : 0.f;
  const float sum = wave_sum(p);
  s_p[lane] = p;
  __builtin_amdgcn_wave_barrier();
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int jj = it * 8 + kg;
    const float pj = jj < ctx ? s_p[jj] : 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      chunk_to_f<T>(L.vv[it][v], f);
#pragma unroll
      for (int e = 0; e < E8; ++e) o[v * E8 + e] += pj * f[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = rows_sum(o[e] + dpp_f<0x128>(o[e]));
  if (kg == 0) store_out8<T>(orow + d8, o, 1.0f / sum);
}

// WAVES items per 64 * WAVES-thread workgroup (the launch site chooses per key source).
template <typename T, typename Keys, bool MASKED, int WAVES, typename Rows = UniformRows>
__global__ __launch_bounds__(64 * WAVES) void vcap_decode_attention_c64_kernel(
    const T* __restrict__ q, const T* __restrict__ kc, const T* __restrict__ vc, Keys keys, T* __restrict__ out, int M,
    int H, Rows rows, KeyMask<MASKED> km) {
  __shared__ __attribute__((aligned(16))) float s_q[WAVES][64];
  __shared__ float s_p[WAVES][64];
  __shared__ int s_a[Keys::kStaged ? WAVES : 1][64];
  const int lane = threadIdx.x & 63, wave = WAVES == 1 ? 0 : threadIdx.x >> 6;
  const int item = blockIdx.x * WAVES + wave;
  if (item >= M * H) return;
  const int m = item / H, h = item - m * H;
  int seq, qpos;
  rows.locate(m, Keys::kSingleQuery, seq, qpos);
  const int ctx = qpos + 1;
  if (!rows.mine(seq, ctx)) return;
  C64Loads<T> L;
  c64_issue<T>(L, q, kc, vc, keys, seq, m, h, H, ctx, s_q[wave], s_a[wave]);
  bool vis = true;
  if constexpr (MASKED) vis = !km.hidden(seq, min(lane, ctx - 1));
  c64_finish<T, Keys::kStaged>(L, s_q[wave], s_p[wave], ctx, out + (long)m * H * 64 + h * 64, vis);
}

// ------------------------------------------------------------------------------------------------
// Launches.  Only what runs is instantiated: paged (general) and contiguous (<= 64) with and without
// the mask, ancestry (both forms) without.
template <typename T, bool MASKED>
static hipError_t launch_decode_attention(const void* q, const void* kc, const void* vc, const DecodeKeys& k, int maxp,
                                          void* out, int M, int H, int S_new, int past, hipStream_t s,
                                          KeyMask<MASKED> km) {
  const bool c64 = past + S_new <= 64;
  auto launch_rows = [&](auto kernel, int waves, auto keys, auto rows) {
    hipLaunchKernelGGL(kernel, dim3((M * H + waves - 1) / waves), dim3(64 * waves), 0, s, (const T*)q, (const T*)kc,
                       (const T*)vc, keys, (T*)out, M, H, rows, km);
    return hipGetLastError();
  };
  auto launch = [&](auto kernel, int waves, auto keys) { return launch_rows(kernel, waves, keys, UniformRows{S_new, past}); };
  if constexpr (!MASKED)
    if (k.row_pos) {
      // ragged prompts: the same four kernels with the row tables.  past + 1 is the launch's longest
      // sequence, k.min_len its shortest: sequences of <= 64 take the <= 64 form, longer ones the general
      // form, as their one-prompt calls do - two launches when the launch holds both
      const bool any64 = k.min_len <= 64, any_long = !c64;
      if (k.row_seq && !k.seq_len) return hipErrorInvalidValue;
      if (any_long && !k.anc && !k.page_table) return hipErrorInvalidValue;
      const TableRows r64{k.row_seq, k.row_pos, k.pos_add, k.seq_len, 0, 64};
      const TableRows rlong{k.row_seq, k.row_pos, k.pos_add, k.seq_len, 64, 0x7fffffff};
      hipError_t err = hipSuccess;
      if (k.anc) {
        const AncestryKeys keys{k.anc, k.anc_ld, maxp};
        if (any64) err = launch_rows(vcap_decode_attention_c64_kernel<T, AncestryKeys, false, 4, TableRows>, 4, keys, r64);
        if (any_long && err == hipSuccess)
          err = launch_rows(vcap_decode_attention_kernel<T, AncestryKeys, false, TableRows>, 4, keys, rlong);
        return err;
      }
      if (any64)
        err = launch_rows(vcap_decode_attention_c64_kernel<T, ContiguousKeys, false, 1, TableRows>, 1,
                          ContiguousKeys{maxp}, r64);
      if (any_long && err == hipSuccess)
        err = launch_rows(vcap_decode_attention_kernel<T, PagedKeys, false, TableRows>, 4,
                          PagedKeys{k.page_table, maxp}, rlong);
      return err;
    }
  if constexpr (!MASKED)
    if (k.anc) {
      const AncestryKeys keys{k.anc, k.anc_ld, maxp};
      return c64 ? launch(vcap_decode_attention_c64_kernel<T, AncestryKeys, false, 4>, 4, keys)
                 : launch(vcap_decode_attention_kernel<T, AncestryKeys, false>, 4, keys);
    }
  if (k.page_table) return launch(vcap_decode_attention_kernel<T, PagedKeys, MASKED>, 4, PagedKeys{k.page_table, maxp});
  if (!c64) return hipErrorInvalidValue;  // a long context needs a page table or an ancestry table
  // one 64-thread workgroup per (row, head): the ~100-200 items of a decode step spread over as
  // many CUs (each item's q / K / V round trip on a CU of its own) instead of 4 per CU
  return launch(vcap_decode_attention_c64_kernel<T, ContiguousKeys, MASKED, 1>, 1, ContiguousKeys{maxp});
}

hipError_t vcap_decode_attention_dispatch(int dt, const void* q, const void* kc, const void* vc, const DecodeKeys& k,
                                          int maxp, void* out, int M, int H, int S_new, int past, hipStream_t s) {
  if (past + S_new > 1024) return hipErrorInvalidValue;
  if (k.anc ? (S_new != 1 || past + 1 > k.anc_ld || k.kmask) : maxp > 64) return hipErrorInvalidValue;
  if (k.row_pos && (S_new != 1 || k.kmask || k.min_len < 1 || k.min_len > past + 1)) return hipErrorInvalidValue;
  const bool bf16 = dt == VCAP_DT_BF16;
  if (!k.kmask) {
    const KeyMask<false> km{};
    return bf16 ? launch_decode_attention<bf16_t>(q, kc, vc, k, maxp, out, M, H, S_new, past, s, km)
                : launch_decode_attention<float>(q, kc, vc, k, maxp, out, M, H, S_new, past, s, km);
  }
  if (k.mask_ld < past + S_new) return hipErrorInvalidValue;
  const KeyMask<true> km{k.kmask, k.mask_ld};
  return bf16 ? launch_decode_attention<bf16_t>(q, kc, vc, k, maxp, out, M, H, S_new, past, s, km)
              : launch_decode_attention<float>(q, kc, vc, k, maxp, out, M, H, S_new, past, s, km);
}
