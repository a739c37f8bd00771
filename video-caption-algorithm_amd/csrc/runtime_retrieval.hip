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

}  // extern "C"
