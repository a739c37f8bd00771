// The C ABI's (include/vcap.h) general entry points: the error string, streams, GEMM, LayerNorm, MX,
// frame and JPEG preprocessing, and the kernel probes.  The ViT schedule is in runtime_vit.hip, the
// GPT-2 decode schedules in runtime_gpt2.hip, their hipGraph cache in graph_cache.hip.
#include <climits>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "runtime_common.h"

thread_local std::string vcap_err;

// ----------------------------------------------------------------------------------- kernel probes
// Live per-site timing for bench.py's roofline: HIP events recorded around every launch of a
// probed site on the caller's stream (no synchronisation; read back after the timed region).
struct Probe {
  std::vector<hipEvent_t> start, stop;
  std::vector<int> rows;   // work size of each launch (GEMM / attention rows), for per-launch pricing
  int used = 0;
  bool on = false;
};

namespace {

std::mutex g_probe_mu;
std::unordered_map<std::string, Probe> g_probes;

Probe* probe_for(const char* site) {
  std::lock_guard<std::mutex> lk(g_probe_mu);
  auto it = g_probes.find(site);
  if (it == g_probes.end() || !it->second.on || it->second.used >= (int)it->second.start.size()) return nullptr;
  return &it->second;
}

// Wait for every recorded launch of `site`, add up its milliseconds (and list them with their rows
// where ms / rows are given: vcap_probe_read_launches, at most `cap`), then disarm the site.
int probe_drain(const char* site, float* ms, int* rows, int cap, float* total_ms, int* launches) {
  std::lock_guard<std::mutex> lk(g_probe_mu);
  auto it = g_probes.find(site);
  *total_ms = 0.f;
  *launches = 0;
  if (it == g_probes.end()) return 0;
  Probe& p = it->second;
  if (p.used > cap) return fail(VCAP_E_ARG, "vcap_probe_read_launches: more launches than cap");
  for (int i = 0; i < p.used; ++i) {
    VCAP_TRY(hipEventSynchronize(p.stop[i]), "hipEventSynchronize");
    float v = 0.f;
    VCAP_TRY(hipEventElapsedTime(&v, p.start[i], p.stop[i]), "hipEventElapsedTime");
    *total_ms += v;
    if (ms) {
      ms[i] = v;
      rows[i] = p.rows[i];
    }
  }
  *launches = p.used;
  p.on = false;
  p.used = 0;
  return 0;
}

}  // namespace

ProbeScope::ProbeScope(const char* site, hipStream_t st, int rows) : p(probe_for(site)), s(st), idx(-1) {
  if (p) {
    idx = p->used++;
    p->rows[idx] = rows;
    (void)hipEventRecord(p->start[idx], s);
  }
}

ProbeScope::~ProbeScope() {
  if (p) (void)hipEventRecord(p->stop[idx], s);
}

// =====================================================================================================
extern "C" {

const char* vcap_last_error(void) { return vcap_err.c_str(); }
int vcap_abi_version(void) { return VCAP_ABI_VERSION; }

int vcap_stream_create_cu_reserved(int reserve_cus, void** stream) {
  if (!stream || reserve_cus < 0) return fail(VCAP_E_ARG, "vcap_stream_create_cu_reserved: bad arguments");
  int dev = 0;
  VCAP_TRY(hipGetDevice(&dev), "hipGetDevice");
  int ncu = 0;
  VCAP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev), "cu count");
  if (reserve_cus >= ncu) return fail(VCAP_E_ARG, "cannot reserve every CU");
  // Clearing the first `reserve_cus` mask bits: with 32 cleared, the stream's workgroups still land on
  // all 8 XCCs and block id % 8 still picks one XCC, so the GEMMs' XCD-aware tile remap
  // holds (r02 per-workgroup stamps with 32 CUs reserved, profiles/r02_encode_alone.txt).
  std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
  for (int c = reserve_cus; c < ncu; ++c) mask[c / 32] |= 1u << (c % 32);
  hipStream_t s = nullptr;
  VCAP_TRY(hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()), "hipExtStreamCreateWithCUMask");
  *stream = (void*)s;
  return 0;
}

int vcap_stream_create_cu_mask(const uint32_t* mask, int words, void** stream) {
  if (!stream || !mask || words <= 0) return fail(VCAP_E_ARG, "vcap_stream_create_cu_mask: bad arguments");
  hipStream_t s = nullptr;
  VCAP_TRY(hipExtStreamCreateWithCUMask(&s, (uint32_t)words, mask), "hipExtStreamCreateWithCUMask");
  *stream = (void*)s;
  return 0;
}

int vcap_stream_destroy(void* stream) {
  VCAP_TRY(hipStreamDestroy((hipStream_t)stream), "hipStreamDestroy");
  return 0;
}

int vcap_set_gemm_policy(int policy) {
  if (policy < 0 || policy > 2) return fail(VCAP_E_ARG, "gemm policy must be 0 (auto), 1 (128x128) or 2 (256x256)");
  vcap_gemm_set_policy(policy);
  return 0;
}

// Both GEMM kernels fetch their operands by 16-byte LDS-DMA (global_load_lds_dwordx4) from A + row * lda + 16-byte
// chunk: every such address is 16-byte aligned exactly when the base is and the row stride is a whole number of
// 16-byte vectors.  A misaligned LDS-DMA source is not something the ISA documentation defines, so it never launches.
static bool gemm_operands_aligned(int in_dtype, const void* A, int64_t lda, const void* W, int64_t ldw) {
  const int64_t ein = 16 / (int64_t)vcap_dt_size(in_dtype);
  return (((uintptr_t)A | (uintptr_t)W) & 15) == 0 && lda % ein == 0 && ldw % ein == 0;
}

int vcap_gemm(int in_dtype, int out_dtype, const void* A, int64_t lda, const void* W, int64_t ldw, void* C,
              int64_t ldc, int M, int N, int K, const float* bias, int act, const float* res, int64_t ldr,
              int res_mode, int G, int Gs, int goff, int roff, void* stream) {
  if (!A || !W || !C || M <= 0 || N <= 0 || K <= 0) return fail(VCAP_E_ARG, "vcap_gemm: bad arguments");
  if (in_dtype != VCAP_DT_F32 && in_dtype != VCAP_DT_BF16 && in_dtype != VCAP_DT_F16)
    return fail(VCAP_E_ARG, "vcap_gemm: operands must be VCAP_DT_F32, VCAP_DT_BF16 or VCAP_DT_F16");
  if (K % vcap_gemm_k_align(in_dtype)) return fail(VCAP_E_UNSUPPORTED, "vcap_gemm: K must be a multiple of the K step");
  if (!gemm_operands_aligned(in_dtype, A, lda, W, ldw))
    return fail(VCAP_E_UNSUPPORTED, "vcap_gemm: A, W 16-byte aligned; lda, ldw in whole 16-byte vectors");
  if (res_mode && !res) return fail(VCAP_E_ARG, "vcap_gemm: residual pointer missing");
  if ((res_mode == 2 || G) && G <= 0) return fail(VCAP_E_ARG, "vcap_gemm: row group G must be > 0");
  if (res_mode && out_dtype != VCAP_DT_F32) return fail(VCAP_E_UNSUPPORTED, "vcap_gemm: residual needs f32 output");
  if (in_dtype == VCAP_DT_F16 && out_dtype != VCAP_DT_F16 && out_dtype != VCAP_DT_F32)
    return fail(VCAP_E_UNSUPPORTED, "vcap_gemm: f16 operands write f16 or f32");
  if (in_dtype == VCAP_DT_BF16 && out_dtype != VCAP_DT_BF16 && out_dtype != VCAP_DT_F32)
    return fail(VCAP_E_UNSUPPORTED, "vcap_gemm: bf16 operands write bf16 or f32");
  if (in_dtype == VCAP_DT_F32 && out_dtype != VCAP_DT_F32)
    return fail(VCAP_E_UNSUPPORTED, "vcap_gemm: f32 operands write f32");
  GemmEpi e{bias, res, (long)ldr, act, res_mode, G, Gs, goff, roff};
  vcap_err.clear();
  VCAP_TRY(vcap_gemm_dispatch(in_dtype, out_dtype, A, lda, W, ldw, C, ldc, M, N, K, e, (hipStream_t)stream),
           "vcap_gemm");
  return 0;
}

int vcap_gemm_splitk(int in_dtype, const void* A, int64_t lda, const void* W, int64_t ldw, float* C, int64_t ldc,
                     int M, int N, int K, const float* bias, int G, int Gs, void* workspace, size_t ws_bytes,
                     int* splits_out, void* stream) {
  if (!A || !W || !C || !bias || !workspace || M <= 0 || N <= 0 || K <= 0 || G < 0 || (G && Gs < G))
    return fail(VCAP_E_ARG, "vcap_gemm_splitk: bad arguments");
  if (in_dtype != VCAP_DT_BF16 && in_dtype != VCAP_DT_F16)
    return fail(VCAP_E_ARG, "vcap_gemm_splitk: operands must be VCAP_DT_BF16 or VCAP_DT_F16");
  if (K % vcap_gemm_k_align(in_dtype)) return fail(VCAP_E_UNSUPPORTED, "vcap_gemm_splitk: K must be a multiple of 64");
  if (!gemm_operands_aligned(in_dtype, A, lda, W, ldw))
    return fail(VCAP_E_UNSUPPORTED, "vcap_gemm_splitk: A, W 16-byte aligned; lda, ldw in whole 16-byte vectors");
  if (N % 4 || ldc % 4 || ((uintptr_t)C & 15) || ((uintptr_t)workspace & 15))
    return fail(VCAP_E_UNSUPPORTED, "vcap_gemm_splitk: N, ldc in whole 16-byte vectors; C and workspace 16-byte aligned");
  if (ws_bytes < (size_t)8 * M * N * sizeof(float)) return fail(VCAP_E_WORKSPACE, "vcap_gemm_splitk: workspace < 8*M*N*4 bytes");
  GemmEpi e{bias, C, (long)ldc, 0, 1, G, Gs, 0, 0, nullptr, nullptr, nullptr, (float*)workspace, ws_bytes};
  vcap_err.clear();
  VCAP_TRY(vcap_gemm_dispatch(in_dtype, VCAP_DT_F32, A, lda, W, ldw, C, ldc, M, N, K, e, (hipStream_t)stream),
           "vcap_gemm_splitk");
  if (splits_out) *splits_out = vcap_gemm_last_splits();
  return 0;
}

int vcap_linear_bias(int dtype, const void* x, const void* w, const float* b, void* y, int rows, int in_features,
                     int out_features, void* stream) {
  return vcap_gemm(dtype, dtype, x, in_features, w, in_features, y, out_features, rows, out_features, in_features, b,
                   0, nullptr, 0, 0, 0, 0, 0, 0, stream);
}

int vcap_layernorm(int out_dtype, const float* x, int64_t ldx, void* y, int64_t ldy, const float* gamma,
                   const float* beta, int rows, int dim, float eps, void* stream) {
  if (!x || !y || rows < 0 || dim <= 0) return fail(VCAP_E_ARG, "vcap_layernorm: bad arguments");
  if ((gamma == nullptr) != (beta == nullptr)) return fail(VCAP_E_ARG, "vcap_layernorm: gamma/beta mismatch");
  VCAP_TRY(vcap_layernorm_dispatch(out_dtype, x, (long)ldx, y, (long)ldy, gamma, beta, rows, dim, eps,
                                   (hipStream_t)stream),
           "vcap_layernorm");
  return 0;
}

size_t vcap_mx_scale_bytes(int rows, int K) {
  if (rows <= 0 || K <= 0 || K % 128) return 0;
  return mx_scale_bytes(rows, K);
}

int vcap_mx_quantize(int in_dtype, const void* x, int64_t ldx, int rows, int K, void* q, uint8_t* scales,
                     void* stream) {
  if (!x || !q || !scales || rows <= 0 || K <= 0 || ldx < K) return fail(VCAP_E_ARG, "vcap_mx_quantize: bad arguments");
  if (in_dtype != VCAP_DT_F32 && in_dtype != VCAP_DT_BF16) return fail(VCAP_E_ARG, "vcap_mx_quantize: in_dtype");
  if (K % 256) return fail(VCAP_E_UNSUPPORTED, "vcap_mx_quantize: K must be a multiple of 256");
  VCAP_TRY(vcap_mx_quantize_dispatch(in_dtype, x, (long)ldx, rows, K, (uint8_t*)q, scales, rows, (hipStream_t)stream),
           "vcap_mx_quantize");
  return 0;
}

int vcap_layernorm_mx(const float* x, int64_t ldx, void* q, uint8_t* scales, const float* gamma, const float* beta,
                      int rows, int dim, float eps, void* stream) {
  if (!x || !q || !scales || rows <= 0 || dim <= 0 || ldx < dim) return fail(VCAP_E_ARG, "vcap_layernorm_mx: bad arguments");
  if ((gamma == nullptr) != (beta == nullptr)) return fail(VCAP_E_ARG, "vcap_layernorm_mx: gamma/beta mismatch");
  if (dim % 256 || dim > 1024) return fail(VCAP_E_UNSUPPORTED, "vcap_layernorm_mx: dim must be 256, 512, 768 or 1024");
  VCAP_TRY(vcap_layernorm_mx_dispatch(x, (long)ldx, (uint8_t*)q, scales, rows, gamma, beta, rows, dim, eps,
                                      (hipStream_t)stream),
           "vcap_layernorm_mx");
  return 0;
}

int vcap_gemm_mx(const void* A, const uint8_t* a_scales, const void* W, const uint8_t* w_scales, int out_dtype,
                 void* C, int64_t ldc, uint8_t* c_scales, int M, int N, int K, const float* bias, int act,
                 const float* res, void* stream) {
  if (!A || !a_scales || !W || !w_scales || !C || M <= 0 || N <= 0 || K <= 0)
    return fail(VCAP_E_ARG, "vcap_gemm_mx: bad arguments");
  if (K % 256) return fail(VCAP_E_UNSUPPORTED, "vcap_gemm_mx: K must be a multiple of 256");
  if (N % 16 || ldc < N || ldc % 16) return fail(VCAP_E_UNSUPPORTED, "vcap_gemm_mx: N and ldc must be multiples of 16");
  if (out_dtype == VCAP_DT_MXFP8) {
    if (act != 1 || !bias || !c_scales || res || N % 128)
      return fail(VCAP_E_UNSUPPORTED, "vcap_gemm_mx: MXFP8 output needs bias + gelu (act=1), c_scales, N % 128 == 0");
    if (reinterpret_cast<uintptr_t>(c_scales) % 8)
      return fail(VCAP_E_ARG, "vcap_gemm_mx: c_scales must be 8-byte aligned");
  } else if (out_dtype != VCAP_DT_BF16 && out_dtype != VCAP_DT_F32) {
    return fail(VCAP_E_ARG, "vcap_gemm_mx: out_dtype");
  }
  if (res && out_dtype != VCAP_DT_F32) return fail(VCAP_E_UNSUPPORTED, "vcap_gemm_mx: residual needs f32 output");
  if (act < 0 || act > 1) return fail(VCAP_E_ARG, "vcap_gemm_mx: act must be 0 or 1");
  GemmEpi e{bias, res, (long)ldc, act, res ? 1 : 0, 0, 0, 0, 0, a_scales, w_scales, c_scales};
  vcap_err.clear();
  VCAP_TRY(vcap_gemm_dispatch(VCAP_DT_MXFP8, out_dtype, A, K, W, K, C, ldc, M, N, K, e, (hipStream_t)stream),
           "vcap_gemm_mx");
  return 0;
}

size_t vcap_frames_workspace_bytes(int n, int in_h, int in_w, int out_h, int out_w) {
  if (n <= 0 || in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0) return 0;
  return vcap_frames_ws_bytes(n, in_h, in_w, out_h, out_w);
}

int vcap_frames_preprocess(const uint8_t* frames, int n, int in_h, int in_w, int out_h, int out_w, const float* mean3,
                           const float* std3, float* out, uint8_t* out_u8, void* workspace, size_t ws_bytes,
                           void* stream) {
  if (!frames || n <= 0 || in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0 || !mean3 || !std3 || (!out && !out_u8) ||
      !workspace)
    return fail(VCAP_E_ARG, "vcap_frames_preprocess: bad arguments");
  if (in_w > 31 * out_w || in_h > 31 * out_h)
    return fail(VCAP_E_UNSUPPORTED, "vcap_frames_preprocess: downscale factor above 31");
  if (ws_bytes < vcap_frames_ws_bytes(n, in_h, in_w, out_h, out_w))
    return fail(VCAP_E_WORKSPACE, "vcap_frames_preprocess: workspace too small");
  VCAP_TRY(vcap_frames_preprocess_dispatch(frames, n, in_h, in_w, out_h, out_w, mean3, std3, out, out_u8, workspace,
                                           (hipStream_t)stream),
           "vcap_frames_preprocess");
  return 0;
}

int vcap_jpeg_probe(const uint8_t* data, size_t len, int* width, int* height, int* comps) {
  if (!data || !len) return fail(VCAP_E_ARG, "vcap_jpeg_probe: bad arguments");
  JpegInfo f;
  std::string e;
  if (int rc = vcap_jpeg_header(data, len, &f, &e)) return fail(rc, "vcap_jpeg_probe: " + e);
  if (width) *width = f.width;
  if (height) *height = f.height;
  if (comps) *comps = f.ncomp;
  return 0;
}

size_t vcap_jpeg_workspace_bytes(const uint8_t* data, size_t len, int n) {
  JpegInfo f;
  std::string e;
  if (!data || !len || n <= 0 || vcap_jpeg_header(data, len, &f, &e)) return 0;
  return vcap_jpeg_ws_bytes(f, n);
}

int vcap_jpeg_decode_batch(const uint8_t* const* data, const size_t* lens, int n, uint8_t* out, void* workspace,
                           size_t ws_bytes, void* stream) {
  if (!data || !lens || n <= 0 || !out || !workspace) return fail(VCAP_E_ARG, "vcap_jpeg_decode_batch: bad arguments");
  for (int i = 0; i < n; ++i)
    if (!data[i] || !lens[i]) return fail(VCAP_E_ARG, "vcap_jpeg_decode_batch: empty image buffer");
  std::string e;
  if (int rc = vcap_jpeg_decode(data, lens, n, out, workspace, ws_bytes, (hipStream_t)stream, &e))
    return fail(rc, "vcap_jpeg_decode_batch: " + e);
  vcap_err.clear();
  return 0;
}

int vcap_probe_enable(const char* site, int max_launches) {
  if (!site || max_launches <= 0) return fail(VCAP_E_ARG, "vcap_probe_enable: bad arguments");
  std::lock_guard<std::mutex> lk(g_probe_mu);
  Probe& p = g_probes[site];
  while ((int)p.start.size() < max_launches) {
    hipEvent_t a, b;
    VCAP_TRY(hipEventCreate(&a), "hipEventCreate");
    VCAP_TRY(hipEventCreate(&b), "hipEventCreate");
    p.start.push_back(a);
    p.stop.push_back(b);
    p.rows.push_back(0);
  }
  p.used = 0;
  p.on = true;
  return 0;
}

int vcap_probe_read_launches(const char* site, float* ms, int* rows, int cap, int* launches) {
  if (!site || !launches || cap < 0 || (cap > 0 && (!ms || !rows)))
    return fail(VCAP_E_ARG, "vcap_probe_read_launches: bad arguments");
  float total;
  return probe_drain(site, ms, rows, cap, &total, launches);
}

int vcap_probe_read(const char* site, float* total_ms, int* launches) {
  if (!site || !total_ms || !launches) return fail(VCAP_E_ARG, "vcap_probe_read: bad arguments");
  return probe_drain(site, nullptr, nullptr, INT_MAX, total_ms, launches);
}

}  // extern "C"

