// agp_ctx.h -- the per-GPU context of the C ABI (agp_ctx), the error-check macros every host function returns through and the
// small launch-geometry helpers.  Host side; the bottom layer of the host headers (agp_*_host.h, agp_svgp_base.h) that agp_capi.hip (one
// translation unit) includes.
#pragma once
#include "../../include/agp_hip.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "agp_chol.h"  // STRACE_SLOTS

using namespace agp;

struct agp_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  int32_t* dag_flags = nullptr;   // tile / x-ready / abort flags of the task-graph factorisation (k_chol_dag), epoch-stamped
  int64_t dag_cap = 0;
  int32_t dag_epoch = 0;
  // sentinel-filled hand-over area of the task graph (set 0; see Dirty below for how it gets refilled)
  void* hset[2] = {nullptr, nullptr};
  size_t hbytes = 0;
  int htype = -1;  // sizeof(T) the sets were filled for
  // lazy refill: a launch leaves its set "dirty"; the next fused kappa' diag(w) kappa launch on the same stream refills it with
  // rider workgroups (no extra launch, stream or event); whoever needs a dirty set before that refills it inline
  struct Dirty {
    bool on = false;
    int64_t used = 0, stride = 0;
    int nb = 0;
  } h_dirty[2];
  int h_step_set = 0;  // the CAVI-step launches with a prologue alternate between the sets and refill each other's (ProArgs::fill)
  void* tri_scratch = nullptr;    // n x n scratch of the recursive-doubling triangular inverse
  size_t tri_bytes = 0;
  // fallback of the task-graph factorisation (k_chol_safe): grid-barrier words, retry counter, number of CUs; once a retry has
  // been seen by the host (any synchronising call) the task graph is not used again on this context
  void* kmm_scratch = nullptr;  // scaled copy + squared norms of the Y side of a kernel matrix whose Y is not a cached Z
  size_t kmm_bytes = 0;
  void* bal_ws = nullptr;       // partial tiles of the balanced triangular product (k_xtx_bal)
  size_t bal_bytes = 0;
  unsigned* safe_bar = nullptr;
  int32_t* safe_retries = nullptr;
  int n_cu = 0;
  bool dag_off = false;
  int64_t dag_retries_seen = 0;
  // probation: after a lost dependency the context factors by plain launches for `dag_cooldown` CAVI steps, then tries the task
  // graph again (whoever shared the GPU may be gone); every further loss makes the next pause four times longer
  int64_t dag_cooldown = 0, dag_backoff = 512;
  // blocked factorisation of large matrices: side stream of the look-ahead (trailing update of the far columns next to the next
  // group's diagonal block and panel), fork / join events, inverses of the current group's diagonal tiles
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  void* chol_li = nullptr;
  size_t chol_li_bytes = 0;
  // split task-graph launches (k_chol_dag ROLE 1 / 2): the chain kernels' own high-priority stream, the word the tile kernel
  // releases them with (signal memory) and the event this context's stream waits on behind every split launch
  hipStream_t chain_stream = nullptr;
  int32_t* chain_go = nullptr;
  int32_t* chain_ctr = nullptr;      // device word: chain workgroups that have exited (DagSync::done); chain_exits = what it will reach
  int32_t chain_exits = 0;
  int chain_state = 0;  // 0 not tried, 1 usable, -1 not available (the two streams do not run kernels side by side) / switched off
  int32_t chain_seq = 0;
  // development aid (builds with -DAGP_STEP_TRACE, run with AGP_STEP_TRACE=<file>): a ring of STRACE_RECS stamp records, one per
  // CAVI-step launch with a prologue (agp_chol.h, STRACE_*), written to the file by agp_ctx_destroy
  unsigned long long* strace = nullptr;
  unsigned long long* strace_last = nullptr;  // the record of the last launch (its deferred fallback stamps into it)
  int64_t strace_n = 0;
};

#ifdef AGP_STEP_TRACE
constexpr int64_t STRACE_RECS = 1024;
static unsigned long long* step_trace_next(agp_ctx* c) {
  static const char* path = getenv("AGP_STEP_TRACE");
  if (!path || !path[0]) return nullptr;
  const size_t bytes = sizeof(unsigned long long) * STRACE_SLOTS * STRACE_RECS;
  if (!c->strace) {
    if (hipMalloc((void**)&c->strace, bytes) != hipSuccess) return c->strace = nullptr;
    (void)hipMemsetAsync(c->strace, 0, bytes, c->stream);
  }
  return c->strace + (c->strace_n++ % STRACE_RECS) * STRACE_SLOTS;
}
static void step_trace_dump(agp_ctx* c) {
  const char* path = getenv("AGP_STEP_TRACE");
  if (!c->strace || !path) return;
  const int64_t n = std::min<int64_t>(c->strace_n, STRACE_RECS);
  std::vector<unsigned long long> h((size_t)(STRACE_SLOTS * STRACE_RECS));
  (void)hipDeviceSynchronize();
  (void)hipMemcpy(h.data(), c->strace, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  if (FILE* f = fopen(path, "wb")) {  // records oldest first: [n, slots] as int64, then n x slots stamps
    const int64_t hdr[2] = {n, STRACE_SLOTS};
    fwrite(hdr, sizeof(hdr), 1, f);
    for (int64_t i = c->strace_n - n; i < c->strace_n; ++i)
      fwrite(h.data() + (i % STRACE_RECS) * STRACE_SLOTS, sizeof(unsigned long long), STRACE_SLOTS, f);
    fclose(f);
  }
  (void)hipFree(c->strace);
  c->strace = nullptr;
}
#else
static unsigned long long* step_trace_next(agp_ctx*) { return nullptr; }
static void step_trace_dump(agp_ctx*) {}
#endif

#define HIPCHK(ctx, expr)                                                                       \
  do {                                                                                          \
    hipError_t _e = (expr);                                                                     \
    if (_e != hipSuccess) {                                                                     \
      (ctx)->err = std::string(#expr) + " : " + hipGetErrorString(_e);                          \
      return AGP_ERR_HIP;                                                                       \
    }                                                                                           \
  } while (0)

#define LAUNCHCHK(ctx)                                                                          \
  do {                                                                                          \
    hipError_t _e = hipGetLastError();                                                          \
    if (_e != hipSuccess) {                                                                     \
      (ctx)->err = std::string("kernel launch : ") + hipGetErrorString(_e) + " @" __FILE_NAME__ ":" + std::to_string(__LINE__); \
      return AGP_ERR_HIP;                                                                       \
    }                                                                                           \
  } while (0)

#define AGPCHK(expr)                   \
  do {                                 \
    agp_status _s = (expr);            \
    if (_s != AGP_OK) return _s;       \
  } while (0)

// Every entry point runs with the ctx's device current and restores the caller's on the way out: the caller's thread may
// have another device selected (two models on two GPUs in one process, torch.cuda.set_device between calls), and a library
// must not change it behind the caller's back.
struct DevGuard {
  int prev = -1;
  bool switched = false;
  explicit DevGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) switched = hipSetDevice(dev) == hipSuccess;
  }
  ~DevGuard() {
    if (switched && prev >= 0) (void)hipSetDevice(prev);
  }
  DevGuard(const DevGuard&) = delete;
  DevGuard& operator=(const DevGuard&) = delete;
};

static inline int64_t rup64(int64_t x) { return (x + 63) / 64 * 64; }
static inline dim3 grid1(int64_t n, int b = 256) { return dim3((unsigned)((n + b - 1) / b)); }
static inline dim3 grid2(int64_t rows, int64_t cols) { return dim3((unsigned)((cols + 15) / 16), (unsigned)((rows + 15) / 16)); }
static const dim3 blk2(16, 16);

template <typename T>
static agp_status dmalloc(agp_ctx* c, T** p, int64_t n) {
  *p = nullptr;
  if (n <= 0) n = 1;
  hipError_t e = hipMalloc((void**)p, (size_t)n * sizeof(T));
  if (e != hipSuccess) {
    c->err = std::string("hipMalloc : ") + hipGetErrorString(e);
    return AGP_ERR_NOMEM;
  }
  return AGP_OK;
}
