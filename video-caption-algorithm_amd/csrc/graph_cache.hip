// Instantiated decode graphs, keyed on everything a replay bakes in (descriptor, parameters,
// buffer addresses, device).  A bounded LRU: a long-running server that hands the decoder new
// buffer addresses cannot grow it without limit.  Each entry remembers an event recorded after
// its latest launch, so an evicted graph is destroyed only once its last replay has finished.
#include <cstdlib>
#include <list>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "runtime_common.h"

namespace {

struct GraphEntry {
  hipGraphExec_t exec = nullptr;
  hipEvent_t done = nullptr;
  std::list<std::string>::iterator lru;
};
std::mutex g_graph_mu;
std::unordered_map<std::string, GraphEntry> g_graphs;
std::list<std::string> g_graph_lru;  // front = most recently used
std::unordered_map<int, hipStream_t> g_capture_streams;

size_t graph_cache_cap() {
  static size_t cap = [] {
    const char* e = std::getenv("VCAP_GRAPH_CACHE_MAX");
    // serving sees one greedy + one beam graph per (batch size, prompt, workspace): 64 entries keep a
    // service whose coalesced batch sizes vary over 1..8 from re-capturing on every call
    long v = e ? std::strtol(e, nullptr, 10) : 64;
    return (size_t)(v < 1 ? 1 : v);
  }();
  return cap;
}

// caller holds g_graph_mu: unlink the least recently used entries down to n and hand them back, so
// the caller destroys them (waiting for their last replay) after releasing the mutex - a wait under
// the lock would stall every decode on other threads / streams
std::vector<GraphEntry> graph_cache_evict_to(size_t n) {
  std::vector<GraphEntry> out;
  while (g_graphs.size() > n && !g_graph_lru.empty()) {
    auto it = g_graphs.find(g_graph_lru.back());
    g_graph_lru.pop_back();
    if (it == g_graphs.end()) continue;
    out.push_back(it->second);
    g_graphs.erase(it);
  }
  return out;
}

// evicted entries, destroyed when this goes out of scope (declared before the lock_guard, so
// after the mutex is released)
struct Evicted {
  std::vector<GraphEntry> v;
  ~Evicted() {
    for (GraphEntry& ge : v) {
      if (ge.done) {
        (void)hipEventSynchronize(ge.done);
        (void)hipEventDestroy(ge.done);
      }
      if (ge.exec) (void)hipGraphExecDestroy(ge.exec);
    }
  }
};

// The descriptor's bytes up to its last field: vcap_gpt2_desc ends in a pointer + a float, so its
// 4 bytes of tail padding (whatever a C caller's stack held) stay out of the key; the int / float
// head is 8 x 4 bytes, so no interior padding precedes the pointers.
static_assert(offsetof(vcap_gpt2_desc, wte) == 8 * sizeof(int), "vcap_gpt2_desc: interior padding");
static_assert(sizeof(vcap_gpt2_layer) == 12 * sizeof(void*), "vcap_gpt2_layer: padding");
static_assert(sizeof(vcap_gen_params) == 8 * sizeof(int) && sizeof(vcap_beam_params) == 10 * sizeof(int),
              "vcap_gen_params / vcap_beam_params: padding");

}  // namespace

void GraphKey::put_desc(const vcap_gpt2_desc* d) {
  put(d, offsetof(vcap_gpt2_desc, screen_bound) + sizeof(d->screen_bound));
  for (int l = 0; l < d->n_layer; ++l) put(&d->layers[l], sizeof(vcap_gpt2_layer));
}

void GraphKey::put_device() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  val(dev);
}

int launch_cached(const std::string& key, hipStream_t s, const std::function<int(hipStream_t)>& issue) {
  Evicted evicted;   // destroyed after the lock is released (declared first)
  std::lock_guard<std::mutex> lk(g_graph_mu);
  auto it = g_graphs.find(key);
  if (it == g_graphs.end()) {
    int dev = 0;
    VCAP_TRY(hipGetDevice(&dev), "hipGetDevice");
    hipStream_t cs = g_capture_streams[dev];
    if (!cs) {
      VCAP_TRY(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking), "hipStreamCreate");
      g_capture_streams[dev] = cs;
    }
    VCAP_TRY(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal), "hipStreamBeginCapture");
    int rc = issue(cs);
    hipGraph_t graph = nullptr;
    hipError_t ec = hipStreamEndCapture(cs, &graph);
    if (rc) {
      if (graph) (void)hipGraphDestroy(graph);
      return rc;
    }
    VCAP_TRY(ec, "hipStreamEndCapture");
    GraphEntry ge;
    hipError_t ei = hipGraphInstantiate(&ge.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    VCAP_TRY(ei, "hipGraphInstantiate");
    if (hipError_t ee = hipEventCreateWithFlags(&ge.done, hipEventDisableTiming)) {
      (void)hipGraphExecDestroy(ge.exec);
      return hip_fail(ee, "hipEventCreate");
    }
    evicted.v = graph_cache_evict_to(graph_cache_cap() - 1);
    g_graph_lru.push_front(key);
    ge.lru = g_graph_lru.begin();
    it = g_graphs.emplace(key, ge).first;
  } else {
    g_graph_lru.splice(g_graph_lru.begin(), g_graph_lru, it->second.lru);
  }
  VCAP_TRY(hipGraphLaunch(it->second.exec, s), "hipGraphLaunch");
  VCAP_TRY(hipEventRecord(it->second.done, s), "hipEventRecord");
  return 0;
}

extern "C" {

void vcap_graph_cache_clear(void) {
  Evicted evicted;
  std::lock_guard<std::mutex> lk(g_graph_mu);
  evicted.v = graph_cache_evict_to(0);
  g_graphs.clear();
  g_graph_lru.clear();
}

int vcap_graph_cache_size(void) {
  std::lock_guard<std::mutex> lk(g_graph_mu);
  return (int)g_graphs.size();
}

}  // extern "C"
