// Private to the host runtime behind the C ABI (runtime.hip, runtime_vit.hip, runtime_gpt2.hip,
// graph_cache.hip): the error plumbing, workspace carving, the probe scope and the graph cache's interface.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <functional>
#include <string>

#include "../../include/vcap.h"
#include "vcap_common.h"
#include "vcap_kernels.h"

extern thread_local std::string vcap_err;   // what vcap_last_error() returns (defined in runtime.hip)

inline int fail(int code, const std::string& msg) {
  vcap_err = msg;
  return code;
}

inline int hip_fail(hipError_t e, const char* where) {
  if (e == hipSuccess) return 0;
  vcap_err = std::string(where) + ": " + hipGetErrorString(e);
  return -(int)e;
}

#define VCAP_TRY(expr, where)                    \
  do {                                           \
    hipError_t _e = (expr);                      \
    if (_e != hipSuccess) return hip_fail(_e, where); \
  } while (0)

inline size_t esize(int dt) { return vcap_dt_size(dt); }
inline size_t mx_scale_bytes(int rows, int K) { return (size_t)(K / 128) * (size_t)((rows + 255) / 256) * 1024; }
inline size_t al(size_t x) { return (x + 255) & ~size_t(255); }

// Hands out 256-byte-aligned pieces of a workspace; over a null base it only adds up, so a size query
// and the launch that carves the same buffers cannot disagree.
struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* b) : base((char*)b) {}
  void* take(size_t bytes) {
    void* p = base ? base + off : nullptr;
    off += al(bytes);
    return p;
  }
};

// what a workspace query returns: the bytes `carve(Carver&)` takes
template <typename F>
size_t carved_bytes(F carve) {
  Carver c(nullptr);
  carve(c);
  return c.off;
}

// Times one launch of a probed site (runtime.hip: vcap_probe_enable / vcap_probe_read*): HIP events
// recorded around it on the caller's stream, no synchronisation.  `site` is read in the constructor only.
struct Probe;
struct ProbeScope {
  Probe* p;
  hipStream_t s;
  int idx;
  ProbeScope(const char* site, hipStream_t st, int rows);
  ~ProbeScope();
};

// ---- runtime_gpt2.hip, for the scoring call's backward (runtime_gpt2_grad.hip)
// the descriptor checks of every GPT-2 entry point (launch: plus the weight pointers a launch dereferences)
int vcap_gpt2_check_desc(const vcap_gpt2_desc* d, bool launch);
struct ScoreForward {   // what the forward leaves in its workspace for the backward
  const float* pmax;    // [B*S][nparts] per 64-column part: max and sum exp(x - max) of the row's logits
  const float* psum;
  int nparts;
};
struct ScoreTailSnap {  // the forward's own att / act bits of the layers >= first_layer, in the decoder dtype
  void* att;            // [n_layer - first_layer][B*S][E]    the attention output (the attn c_proj's input)
  void* act;            // [n_layer - first_layer][B*S][4E]   gelu_new(c_fc) (the mlp c_proj's input)
  int first_layer;
};
int vcap_score_forward(const vcap_gpt2_desc* d, const float* embeds, int B, int S, const uint8_t* key_mask,
                       const int* targets, float* logits_out, float* logprob_out, float* loss_out, void* workspace,
                       float* snap, hipStream_t s, ScoreForward* out, const ScoreTailSnap* tail = nullptr);

// ---- runtime_text.hip, for the text tower's backward (runtime_text_grad.hip)
int vcap_text_limits(const vcap_text_desc* d, int B, int L, const char* who);
int vcap_text_check_pointers(const vcap_text_desc* d, const void* workspace);
struct TextSnap {   // what the forward keeps for the backward, layer-major (M = B * L rows, T = the operand dtype)
  float* x;         // [n_layer][4][M][E] f32 stream: layer input, pre-LN1 sum, LN1 output, pre-LN2 sum
  char* qkv;        // [n_layer][M][3E] T
  char* attn;       // [n_layer][M][E] T
  char* act;        // [n_layer][M][F] T
};
int vcap_text_forward(const vcap_text_desc* d, const int* ids, int B, int L, float* out, float* hidden_out,
                      void* workspace, const TextSnap* snap, hipStream_t s);

// ---- runtime_vit.hip, for the encoder's backward (runtime_vit_grad.hip)
int vcap_vit_check(const vcap_vit_desc* d);   // the descriptor limits of every ViT entry point
struct VitSnap {   // what the forward keeps of its last n_tail blocks, block-major (M = B*T*tokens rows, T = operand dtype)
  int n_tail;
  float* x0;       // [n_tail][M][D] f32 stream at the block input
  float* x1;       // [n_tail][M][D] f32 stream after the attention residual (the last block: its B*T CLS rows, compact)
  char* qkv;       // [n_tail][M][3D] T
  char* attn;      // [n_tail][M][D] T (the last block: [B*T][D])
  char* act;       // [n_tail][M][mlp] T (the last block: [B*T][mlp])
  // set by the forward: pieces of its workspace - the final stream, the LayerNorm output buffer (free after the
  // forward) and the im2col patches (intact when every block is kept)
  float* x;
  void* xn;
  void* patches;
};
int vcap_vit_forward(const vcap_vit_desc* d, const vcap_prefix_desc* pd, const float* frames, int B, int T,
                     float* enc_out, float* prefix_out, void* workspace, VitSnap* snap, hipStream_t s);

// ---- graph_cache.hip
// Bytes of everything a captured decode bakes in; two calls replay one graph only if their keys are equal.
struct GraphKey {
  std::string k;
  explicit GraphKey(const char* tag = "") : k(tag) {}
  void put(const void* p, size_t n) { k.append((const char*)p, n); }
  template <typename T>
  void val(const T& v) { put(&v, sizeof(v)); }
  void put_desc(const vcap_gpt2_desc* d);   // the descriptor without its tail padding, then every layer
  void put_device();                        // the current device
};

// Replay the graph cached under `key` on s, capturing `issue(capture_stream)` into it first if absent.
int launch_cached(const std::string& key, hipStream_t s, const std::function<int(hipStream_t)>& issue);
