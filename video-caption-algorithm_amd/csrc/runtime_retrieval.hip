// The C ABI's (include/vcap.h) video-retrieval entry points: argument checks and workspace sizing in
// front of the kernels of retrieval.hip.  Every refusal returns before the first launch.
#include <algorithm>

#include "runtime_common.h"

namespace {

bool ip_dtype_ok(int dt) { return dt == VCAP_DT_F32 || dt == VCAP_DT_BF16; }

// the limits of vcap_ip_search (include/vcap.h); 0 when inside them
int ip_limits(int64_t n, int dim, int nq, int k, const char* who) {
  if (n < 0 || dim < 0 || nq < 0 || k < 0) return fail(VCAP_E_ARG, std::string(who) + ": negative size");
  if (dim % 64 || dim < 64 || dim > 1024)
    return fail(VCAP_E_UNSUPPORTED, std::string(who) + ": dim must be a multiple of 64 in 64..1024");
  if (k < 1 || k > kIpMaxK) return fail(VCAP_E_UNSUPPORTED, std::string(who) + ": k must be in 1..128");
  if (nq < 1 || nq > 64 || nq * dim > kIpMaxQueryFloats)
    return fail(VCAP_E_UNSUPPORTED, std::string(who) + ": nq must be in 1..64 with nq * dim <= 16384");
  if (n > 0x7FFFFFFFLL) return fail(VCAP_E_UNSUPPORTED, std::string(who) + ": n must be below 2^31 rows");
  return 0;
}

size_t ip_ws_bytes(int64_t n, int dim, int nq, int k) {
  const int64_t slabs = (n + kIpSlabRows - 1) / kIpSlabRows;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(kIpMaxWorkgroups, slabs));
  const int pass = std::min(nq, vcap_ip_search_pass_tiles(dim) * 16);
  return al((size_t)grid * pass * vcap_ip_search_cap(k) * sizeof(uint64_t));
}

// ---- IVF-Flat (csrc/ivf.hip)
int ivf_dim_ok(int dim, const char* who) {
  if (dim % 64 || dim < 64 || dim > 1024)
    return fail(VCAP_E_UNSUPPORTED, std::string(who) + ": dim must be a multiple of 64 in 64..1024");
  return 0;
}

int ivf_nlist_ok(int64_t nlist, const char* who) {
  if (nlist < 1 || nlist > kIvfMaxLists)
    return fail(VCAP_E_UNSUPPORTED, std::string(who) + ": nlist must be in 1..1048576");
  return 0;
}

// the limits of vcap_ivf_search (include/vcap.h); 0 when inside them
int ivf_limits(int64_t ntotal, int64_t nlist, int64_t max_list_len, int dim, int nq, int nprobe, int k, const char* who) {
  if (nlist < 0 || max_list_len < 0 || nprobe < 0) return fail(VCAP_E_ARG, std::string(who) + ": negative size");
  if (int rc = ip_limits(ntotal, dim, nq, k, who)) return rc;
  if (nprobe < 1 || nprobe > kIvfMaxProbe)
    return fail(VCAP_E_UNSUPPORTED, std::string(who) + ": nprobe must be in 1..128");
  if (int rc = ivf_nlist_ok(nlist, who)) return rc;
  if (max_list_len > ntotal) return fail(VCAP_E_ARG, std::string(who) + ": max_list_len exceeds ntotal");
  return 0;
}

// the pieces of vcap_ivf_search's workspace, in carving order
struct IvfWs {
  void* coarse;
  long long* probes;
  float* probe_scores;
  void* keys;
};
IvfWs ivf_carve(Carver& c, int64_t nlist, int64_t max_list_len, int dim, int nq, int nprobe, int k) {
  IvfWs w;
  const int64_t slices = (max_list_len + kIvfSliceRows - 1) / kIvfSliceRows;
  w.coarse = c.take(ip_ws_bytes(nlist, dim, nq, nprobe));
  w.probes = (long long*)c.take((size_t)nq * nprobe * sizeof(long long));
  w.probe_scores = (float*)c.take((size_t)nq * nprobe * sizeof(float));
  w.keys = c.take((size_t)std::max<int64_t>(1, slices) * nprobe * nq * k * sizeof(uint64_t));
  return w;
}

}  // namespace

extern "C" {

int vcap_l2_normalize(const float* x, int64_t ldx, float* y, int64_t ldy, int rows, int dim, float eps, int eps_mode,
                      void* stream) {
  if (!x || !y || rows < 0 || dim <= 0 || ldx < dim || ldy < dim)
    return fail(VCAP_E_ARG, "vcap_l2_normalize: bad arguments");
  if (eps_mode != 0 && eps_mode != 1)
    return fail(VCAP_E_ARG, "vcap_l2_normalize: eps_mode must be 0 (max(norm, eps)) or 1 (norm + eps)");
  VCAP_TRY(vcap_l2_normalize_dispatch(x, (long)ldx, y, (long)ldy, rows, dim, eps, eps_mode, (hipStream_t)stream),
           "vcap_l2_normalize");
  return 0;
}

int vcap_ip_index_convert(const float* x, int64_t ldx, int rows, int dim, int storage_dtype, void* dst, void* stream) {
  if (!x || !dst || rows < 0 || dim <= 0 || ldx < dim) return fail(VCAP_E_ARG, "vcap_ip_index_convert: bad arguments");
  if (!ip_dtype_ok(storage_dtype))
    return fail(VCAP_E_ARG, "vcap_ip_index_convert: storage_dtype must be VCAP_DT_F32 or VCAP_DT_BF16");
  if (dim % 4 || ldx % 4 || ((uintptr_t)x & 15) || ((uintptr_t)dst & 15))
    return fail(VCAP_E_UNSUPPORTED, "vcap_ip_index_convert: dim and ldx in whole 16-byte vectors; x and dst 16-byte aligned");
  VCAP_TRY(vcap_ip_convert_dispatch(storage_dtype, x, (long)ldx, rows, dim, dst, (hipStream_t)stream),
           "vcap_ip_index_convert");
  return 0;
}

size_t vcap_ip_search_workspace_bytes(int64_t n, int dim, int nq, int k) {
  if (ip_limits(n, dim, nq, k, "vcap_ip_search_workspace_bytes")) return 0;
  return ip_ws_bytes(n, dim, nq, k);
}

int vcap_ip_search_slab_rows(void) { return kIpSlabRows; }

int vcap_ip_search_workgroups(int64_t n, int max_blocks) {
  if (n < 0 || max_blocks < 0) return fail(VCAP_E_ARG, "vcap_ip_search_workgroups: negative size");
  return vcap_ip_search_grid((long)n, max_blocks);
}

int vcap_ip_search(int storage_dtype, const void* db, int64_t n, int dim, const float* queries, int nq, int k,
                   float* out_scores, int64_t* out_ids, void* workspace, size_t ws_bytes, int max_blocks,
                   void* stream) {
  if (!queries || !out_scores || !out_ids || !workspace || (!db && n > 0))
    return fail(VCAP_E_ARG, "vcap_ip_search: null pointer");
  if (max_blocks < 0) return fail(VCAP_E_ARG, "vcap_ip_search: negative size");
  if (!ip_dtype_ok(storage_dtype))
    return fail(VCAP_E_ARG, "vcap_ip_search: storage_dtype must be VCAP_DT_F32 or VCAP_DT_BF16");
  if (int rc = ip_limits(n, dim, nq, k, "vcap_ip_search")) return rc;
  if (((uintptr_t)db & 15) || ((uintptr_t)queries & 15) || ((uintptr_t)workspace & 7))
    return fail(VCAP_E_UNSUPPORTED, "vcap_ip_search: db and queries must be 16-byte aligned, the workspace 8-byte");
  if (ws_bytes < ip_ws_bytes(n, dim, nq, k))
    return fail(VCAP_E_WORKSPACE, "vcap_ip_search: workspace too small (vcap_ip_search_workspace_bytes)");
  VCAP_TRY(vcap_ip_search_dispatch(storage_dtype, db, (long)n, dim, queries, nq, k, out_scores, (long long*)out_ids,
                                   workspace, max_blocks, (hipStream_t)stream),
           "vcap_ip_search");
  return 0;
}

int vcap_ivf_slice_rows(void) { return kIvfSliceRows; }
int vcap_ivf_chunk_rows(void) { return kIvfChunkRows; }

int vcap_ivf_assign(const float* x, int64_t ldx, int64_t n, const float* centroids, int nlist, int dim, int32_t* assign,
                    float* score, void* stream) {
  if (!x || !centroids || !assign) return fail(VCAP_E_ARG, "vcap_ivf_assign: null pointer");
  if (n < 0 || nlist < 0 || dim < 0 || ldx < dim) return fail(VCAP_E_ARG, "vcap_ivf_assign: bad sizes");
  if (int rc = ivf_dim_ok(dim, "vcap_ivf_assign")) return rc;
  if (int rc = ivf_nlist_ok(nlist, "vcap_ivf_assign")) return rc;
  if (n > 0x7FFFFFFFLL) return fail(VCAP_E_UNSUPPORTED, "vcap_ivf_assign: n must be below 2^31 rows");
  if (ldx % 4 || ((uintptr_t)x & 15) || ((uintptr_t)centroids & 15))
    return fail(VCAP_E_UNSUPPORTED, "vcap_ivf_assign: ldx in whole 16-byte vectors; x and centroids 16-byte aligned");
  VCAP_TRY(vcap_ivf_assign_dispatch(x, (long)ldx, (long)n, centroids, nlist, dim, assign, score, (hipStream_t)stream),
           "vcap_ivf_assign");
  return 0;
}

size_t vcap_ivf_centroid_update_workspace_bytes(int64_t n, int nlist, int dim) {
  if (n < 0 || n > 0x7FFFFFFFLL || ivf_dim_ok(dim, "vcap_ivf_centroid_update_workspace_bytes") ||
      ivf_nlist_ok(nlist, "vcap_ivf_centroid_update_workspace_bytes"))
    return 0;
  return al((size_t)vcap_ivf_update_slots((long)n, nlist) * dim * sizeof(float));
}

int vcap_ivf_centroid_update(const float* x, int64_t ldx, int64_t n, int dim, const int64_t* order,
                             const int64_t* offsets, int nlist, const float* prev, float* out, void* workspace,
                             size_t ws_bytes, void* stream) {
  const char* who = "vcap_ivf_centroid_update";
  if (!x || !order || !offsets || !prev || !out || !workspace) return fail(VCAP_E_ARG, std::string(who) + ": null pointer");
  if (n < 0 || nlist < 0 || dim < 0 || ldx < dim) return fail(VCAP_E_ARG, std::string(who) + ": bad sizes");
  if (int rc = ivf_dim_ok(dim, who)) return rc;
  if (int rc = ivf_nlist_ok(nlist, who)) return rc;
  if (n > 0x7FFFFFFFLL) return fail(VCAP_E_UNSUPPORTED, std::string(who) + ": n must be below 2^31 rows");
  if (ldx % 4 || ((uintptr_t)x & 15) || ((uintptr_t)workspace & 15))
    return fail(VCAP_E_UNSUPPORTED, std::string(who) + ": ldx in whole 16-byte vectors; x and the workspace 16-byte aligned");
  if (ws_bytes < vcap_ivf_centroid_update_workspace_bytes(n, nlist, dim))
    return fail(VCAP_E_WORKSPACE, std::string(who) + ": workspace too small (vcap_ivf_centroid_update_workspace_bytes)");
  VCAP_TRY(vcap_ivf_centroid_update_dispatch(x, (long)ldx, (long)n, dim, (const long long*)order,
                                             (const long long*)offsets, nlist, prev, out, 1e-12f, (float*)workspace,
                                             (hipStream_t)stream),
           who);
  return 0;
}

size_t vcap_ivf_search_workspace_bytes(int nlist, int64_t max_list_len, int dim, int nq, int nprobe, int k) {
  // ntotal is not an argument: any list length below 2^31 is sized
  if (max_list_len > 0x7FFFFFFFLL ||
      ivf_limits(std::max<int64_t>(0, max_list_len), nlist, max_list_len, dim, nq, nprobe, k, "vcap_ivf_search_workspace_bytes"))
    return 0;
  return carved_bytes([&](Carver& c) { ivf_carve(c, nlist, max_list_len, dim, nq, nprobe, k); });
}

int vcap_ivf_search(int storage_dtype, const void* rows, const int64_t* ids, const int64_t* offsets, int64_t ntotal,
                    const float* centroids, int nlist, int64_t max_list_len, int dim, const float* queries, int nq,
                    int nprobe, int k, float* out_scores, int64_t* out_ids, int64_t* out_probes, void* workspace,
                    size_t ws_bytes, int max_blocks, void* stream) {
  if (!offsets || !centroids || !queries || !out_scores || !out_ids || !workspace || ((!rows || !ids) && ntotal > 0))
    return fail(VCAP_E_ARG, "vcap_ivf_search: null pointer");
  if (max_blocks < 0) return fail(VCAP_E_ARG, "vcap_ivf_search: negative size");
  if (!ip_dtype_ok(storage_dtype))
    return fail(VCAP_E_ARG, "vcap_ivf_search: storage_dtype must be VCAP_DT_F32 or VCAP_DT_BF16");
  if (int rc = ivf_limits(ntotal, nlist, max_list_len, dim, nq, nprobe, k, "vcap_ivf_search")) return rc;
  if (((uintptr_t)rows & 15) || ((uintptr_t)centroids & 15) || ((uintptr_t)queries & 15) || ((uintptr_t)workspace & 15))
    return fail(VCAP_E_UNSUPPORTED, "vcap_ivf_search: rows, centroids, queries and the workspace must be 16-byte aligned");
  if (ws_bytes < carved_bytes([&](Carver& c) { ivf_carve(c, nlist, max_list_len, dim, nq, nprobe, k); }))
    return fail(VCAP_E_WORKSPACE, "vcap_ivf_search: workspace too small (vcap_ivf_search_workspace_bytes)");
  Carver c(workspace);
  const IvfWs w = ivf_carve(c, nlist, max_list_len, dim, nq, nprobe, k);
  VCAP_TRY(vcap_ivf_search_dispatch(storage_dtype, rows, (const long long*)ids, (const long long*)offsets, (long)ntotal,
                                    centroids, nlist, (long)max_list_len, dim, queries, nq, nprobe, k, out_scores,
                                    (long long*)out_ids, out_probes ? (long long*)out_probes : w.probes,
                                    w.probe_scores, w.coarse, w.keys, max_blocks, (hipStream_t)stream),
           "vcap_ivf_search");
  return 0;
}

}  // extern "C"
