// agp_chol_host.h -- host driver of the Cholesky factorisation (kernels: agp_chol.h): the task-graph launch (k_chol_dag, merged or
// split into chain kernel + tile kernel) with its hand-over sets, flags and in-stream fallback, and the plain per-column / blocked
// launches.  Entry points: potrf_fused (one problem, PotrfReq), potrf_dag_batch / potrf_fused_batch (nb problems of one shape).
#pragma once
#include <cmath>
#include "agp_ctx.h"
#include "agp_linalg.h"

// ---- linear-algebra drivers on padded matrices ---------------------------------------------------------------
// Cholesky (lower, in place; diagonal factors in Dg) of the n x n (n = nt*64) matrix A with `ne` extension row blocks
static agp_status tri_scratch_ensure(agp_ctx* c, size_t need) {
  if (c->tri_bytes < need) {
    if (c->tri_scratch) {
      (void)hipStreamSynchronize(c->stream);
      (void)hipFree(c->tri_scratch);
    }
    c->tri_scratch = nullptr;
    c->tri_bytes = 0;
    if (hipMalloc(&c->tri_scratch, need) != hipSuccess) return AGP_ERR_NOMEM;
    c->tri_bytes = need;
  }
  return AGP_OK;
}

// E <- E L^-T (augmented Cholesky): nt launches of k_chol_step; do_x adds X = L^-1 (one extra row launch per column).
// X = L^-1 (all off-diagonal tiles) from L and the diagonal inverses already in X: recursive doubling, 2 launches per level
template <typename T>
static agp_status trtri_levels(agp_ctx* c, const T* A, int64_t ld, T* X, int64_t ldx, int64_t nt) {
  if (nt <= 1) return AGP_OK;
  const int64_t n = nt * TILE;
  AGPCHK(tri_scratch_ensure(c, sizeof(T) * (size_t)n * (size_t)n));
  T* S = (T*)c->tri_scratch;
  for (int64_t bs = 1; bs < nt; bs *= 2) {
    const int64_t pairs = (nt + 2 * bs - 1) / (2 * bs);
    dim3 g((unsigned)bs, (unsigned)bs, (unsigned)pairs);
    hipLaunchKernelGGL((k_trtri_level<T>), g, dim3(NTHREADS), 0, c->stream, A, ld, X, ldx, S, n, nt, bs, 0);
    hipLaunchKernelGGL((k_trtri_level<T>), g, dim3(NTHREADS), 0, c->stream, A, ld, X, ldx, S, n, nt, bs, 1);
  }
  LAUNCHCHK(c);
  return AGP_OK;
}

// hand-over area for the next task-graph launch (`elems` elements of T): waits for the pending refill of the set, returns it;
// dag_handover_release() schedules the refill behind the launch
template <typename T>
static agp_status dag_handover_acquire(agp_ctx* c, int64_t elems, int set, T** out) {
  const size_t need = sizeof(T) * (size_t)elems;
  if (c->hbytes < need || c->htype != (int)sizeof(T)) {
    (void)hipStreamSynchronize(c->stream);
    for (int q = 0; q < 2; ++q) {
      if (c->hset[q]) (void)hipFree(c->hset[q]);
      c->hset[q] = nullptr;
      c->h_dirty[q].on = false;
    }
    c->hbytes = 0;
    const size_t cap = need + need / 4;
    c->hbytes = cap;
    c->htype = (int)sizeof(T);
  }
  if (!c->hset[set]) {  // set 1 only exists once a step launch with a prologue asks for it (they alternate between the sets)
    if (hipMalloc(&c->hset[set], c->hbytes) != hipSuccess) return AGP_ERR_NOMEM;
    hipLaunchKernelGGL((k_fill_sent<T>), dim3(2048), dim3(256), 0, c->stream, (T*)c->hset[set], (int64_t)(c->hbytes / sizeof(T)),
                       (int64_t)0);
    c->h_dirty[set].on = false;
  }
  if (c->h_dirty[set].on) {  // nobody refilled it in passing: do it now, on this stream
    const auto& d = c->h_dirty[set];
    hipLaunchKernelGGL((k_fill_sent<T>), dim3((unsigned)std::max<int64_t>(1, 512 / d.nb), (unsigned)d.nb), dim3(256), 0, c->stream,
                       (T*)c->hset[set], d.used, d.stride);
    c->h_dirty[set].on = false;
  }
  *out = (T*)c->hset[set];
  return AGP_OK;
}
template <typename T>
static agp_status dag_handover_release(agp_ctx* c, int64_t used, int64_t stride, int nb, int set) {
  // what the launch could have written (the first `used` elements of each of the nb problem regions) must hold the sentinel
  // again before the set's next use: left to the next fused syrk launch (riders) or, failing that, to the next acquire
  c->h_dirty[set] = {true, used, stride, nb};
  return AGP_OK;
}

// One-launch task graph (k_chol_dag) or one launch per block column (k_chol_step)?  Measured on MI355X, whole CAVI step:
// m = 1024 f64 0.39 vs 0.52 ms, m = 2048 f32 0.80 vs 1.05 ms, m = 4096 f64 11.6 vs 8.3 ms -- the task graph removes launch
// gaps and re-reads from the latency-bound chain, but its tiles stream their operands past the L2s (coherent loads), which
// costs more than it saves once the trailing updates dominate.  AGP_CHOL_DAG=0 / 1 forces one or the other.
// Column bound: the chain of a task graph waits for feeder tiles with HIGHER workgroup indices -- tile (k+1, k) in block column k
// and tile (k+1, k+1), the first workgroup of column k + 1.  Progress does not depend on them being resident early: the chain
// publishes X_k before it blocks on them (k_chol_dag, "late_feed"), so every resident workgroup -- all of them belong to block
// columns <= k of their problem -- can finish on what the chains have published, retires, and the in-order dispatch reaches the
// feeders.  (Rounds 1-2 published X_k after that wait and therefore needed a whole block column of every problem resident,
// nb * (nt + ne + 1) <= 208; 8 problems of 34 tiles stalled.)  What remains is a performance matter: a feeder that gets its slot only
// when the column before it retires applies its k pending updates on the chain's critical path.  Up to 288 tiles per column of all
// problems the launch is still well ahead of per-column launches (8 x 34: 0.62 ms against 2 x 0.40 ms for 4 + 4).
constexpr int64_t DAG_MAX_NT = 32, DAG_MAX_COLUMN_TILES = 288;
static bool chol_use_dag(const agp_ctx* c, int64_t nt, int64_t ne = 0, int64_t nb = 1) {
  static const int v = []() {
    const char* e = getenv("AGP_CHOL_DAG");
    return e ? (e[0] == '0' ? 0 : 1) : -1;
  }();
  if (c->dag_off) return false;  // a lost dependency was seen on this context (two processes sharing the device): stay safe
  if (nb * (nt + ne + 1) > DAG_MAX_COLUMN_TILES) return false;
  return v < 0 ? nt <= DAG_MAX_NT : v == 1;
}

__global__ void k_set_i32(int32_t* p, int32_t v) { *p = v; }
// ... visible to a polling kernel of another stream (signal memory, system scope)
__global__ void k_set_sig(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
// ... and the arrival word of a column group of the all-reduced statistics (comm_allreduce_groups): the collective's kernel before
// this one on the same stream has ended, i.e. its writes are in memory
__global__ void k_set_arrive(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT); }


// grid-barrier words, retry counter and the CU count of the fallback (allocated on first use)
template <typename T>
static agp_status ensure_safe_words(agp_ctx* c) {
  if (!c->safe_bar) {
    if (hipMalloc((void**)&c->safe_bar, 2 * sizeof(unsigned)) != hipSuccess) return AGP_ERR_NOMEM;
    if (hipMalloc((void**)&c->safe_retries, sizeof(int32_t)) != hipSuccess) return AGP_ERR_NOMEM;
    HIPCHK(c, hipMemsetAsync(c->safe_bar, 0, 2 * sizeof(unsigned), c->stream));
    HIPCHK(c, hipMemsetAsync(c->safe_retries, 0, sizeof(int32_t), c->stream));
    hipDeviceProp_t pr;
    HIPCHK(c, hipGetDeviceProperties(&pr, c->device));
    c->n_cu = pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 64;
  }
  return AGP_OK;
}

// Workgroups the grid-barrier fallback may count on being resident together.  One per CU -- minus the CUs a chain kernel of the
// NEXT split launch may be sitting on: with the host ahead, that kernel is already in flight on its own stream, polls for a tile
// kernel that is enqueued BEHIND the fallback, and holds most of its CU's LDS while it does (a fallback workgroup cannot share the
// CU).  A fallback grid of n_cu workgroups would then wait at its first barrier for a workgroup that can never be placed.
static int64_t safe_grid_cap(const agp_ctx* c) {
  // test hook (AGP_DAG_TEST_OVERSUBSCRIBE=1, with AGP_DAG_TEST_ABORT=1): a fallback grid that CANNOT be resident at once (four
  // workgroups of ~110 KB LDS per CU), i.e. the situation the bounded grid barrier exists for -- the step must end in status -3
  // (AGP_ERR_HIP from agp_svgp_check_status) after the barrier's limit instead of hanging (tests/test_gpu_round6.py)
  static const bool over = []() {
    const char* e = getenv("AGP_DAG_TEST_OVERSUBSCRIBE");
    return e && e[0] == '1';
  }();
  if (over) return 4 * (int64_t)c->n_cu;
  return std::max<int64_t>(1, (int64_t)c->n_cu - (c->chain_state == 1 ? CHOL_MAXB : 0));
}
// the fallback behind a task-graph launch (see k_chol_safe): one launch that returns at once unless the latch reads -1
template <typename T>
static agp_status launch_chol_safe(agp_ctx* c, const CholBatch<T>& bt, const SafeSrc<T>& src, int nb, int64_t ld, int64_t ldx,
                                   int64_t lde, int64_t ne, int64_t nt, int32_t* info_dev, int64_t nvalid) {
  AGPCHK(ensure_safe_words<T>(c));
  // one workgroup per CU at most (each needs ~110 KB of LDS, so one fits per CU): all of them become resident, whatever else runs
  const int64_t most = (nt + ne + nt * (nt + 1) / 2 + ne * nt) * nb;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(safe_grid_cap(c), most));
  hipLaunchKernelGGL((k_chol_safe<T>), dim3(grid), dim3(CHOL_THREADS), 0, c->stream, bt, src, nb, ld, ldx, lde, ne, nt, info_dev,
                     nvalid, c->safe_bar, c->safe_retries);
  LAUNCHCHK(c);
  return AGP_OK;
}
// The kernel behind the task graph of a single-latent CAVI step: the fallback of k_chol_safe (a no-op unless the latch reads -1)
// and then the row statistics + local update, in ONE launch -- the separate k_chol_safe launch cost the step ~5 us of kernel and a
// launch gap on its critical path.  grid <= n_cu workgroups of 512 threads (all resident: the fallback uses grid barriers); the
// rows are taken wave by wave, grid-stride.
template <typename T>
__global__ __launch_bounds__(CHOL_THREADS) void k_safe_rowstats(CholBatch<T> bt, SafeSrc<T> src, int64_t ld, int64_t ldx, int64_t lde,
                                                                int64_t ne, int64_t nt, int32_t* __restrict__ info, int64_t nvalid,
                                                                unsigned* __restrict__ bar, int32_t* __restrict__ retries,
                                                                int64_t B, int nslices, RowstatsBatch<T> rb, int64_t ldp,
                                                                int64_t ldw, int64_t cols, T jitter, T rho, LikParams<T> lp,
                                                                const T* __restrict__ y, const int64_t* __restrict__ idx,
                                                                T* __restrict__ Kt, T* __restrict__ muf, T* __restrict__ varf,
                                                                T* __restrict__ cb, T* __restrict__ theta, T* __restrict__ r,
                                                                T* __restrict__ w, int* __restrict__ flags,
                                                                const T* __restrict__ lam, T* __restrict__ gamma,
                                                                int rows_done = 0, const int32_t* __restrict__ pf_word = nullptr,
                                                                int32_t pf_want = 0, const T* __restrict__ s00_kap = nullptr,
                                                                int64_t s00_ldk = 0, int64_t s00_K = 0,
                                                                const T* __restrict__ s00_w = nullptr, T* __restrict__ pre = nullptr,
                                                                unsigned long long* trace = nullptr) {
  __shared__ __attribute__((aligned(16))) T sm[3 * TILE * LDP];
  __shared__ __attribute__((aligned(16))) T sc[SC_ELEMS];
  __shared__ T piv[TILE];
#ifdef AGP_STEP_TRACE
  if (trace && threadIdx.x == 0 && blockIdx.x < 256) trace[STRACE_SAFE0 + blockIdx.x] = wall_clock64();
  StraceExit strace_exit{(trace && blockIdx.x < 256) ? trace + STRACE_SAFE1 + blockIdx.x : nullptr};
#else
  (void)trace;
#endif
  const bool ran = chol_safe_body<T>(bt, src, 1, ld, ldx, lde, ne, nt, info, nvalid, bar, retries, sm, sc, piv);
  // (after a fallback the last grid barrier of the column loop has made every workgroup's tiles visible)
  // rows_done (round 3): the task-graph launch finished its rows itself (EpiArgs, agp_chol.h) -- unless it was aborted and re-run here
  if (ran || !rows_done) {
    const int64_t wpb = CHOL_THREADS / 64, nwave = (int64_t)gridDim.x * wpb;
    for (int64_t i = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6); i < B; i += nwave)
      rowstats_row<T>(i, threadIdx.x & 63, 0, B, nslices, rb, ldp, ldw, cols, jitter, rho, lp, y, idx, Kt, muf, varf, cb, theta, r,
                      w, (int64_t)0, flags, lam, gamma);
  }
  // pre: the first three tiles of S = kappa' diag(w) kappa of the pending natural-gradient step (kappa s00_kap, weights s00_w = the
  // w of the launch in front) for the head of the next launch (ProArgs::pre).  Not where this launch re-ran the fallback: its rows
  // above are not visible to the other workgroups yet, and the next launch's three tiles form their products themselves
  if (pro_pre_on<T>() && pre) {
    if (!ran) pro_pre_prepare<T>(s00_kap, s00_ldk, s00_K, s00_w, pre, sm);
    if (blockIdx.x == 0 && threadIdx.x == 0) pre[PRO_PRE_VALID] = ran ? T(0) : T(1);
  }
  // pf_word (round 3): this launch was deferred to the head of the NEXT step and also carries that step's wait for its look-ahead
  // (one wave polls the look-ahead's "done" word; in the steady state it is set long before)
  if (pf_word && blockIdx.x == 0 && threadIdx.x == 0) {
    long spins = 0;
    while ((int32_t)(__hip_atomic_load(pf_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - pf_want) < 0) {
      __builtin_amdgcn_s_sleep(8);
      if (++spins > (1L << 27)) {
        atomicExch(info, -2);
        break;
      }
    }
  }
}

// The same for the launch behind materialize() (the factorisation of -2 eta2 with its inverse and Sigma = X' X, round 5): the
// fallback, then mu = Sigma eta1 and v = X eta1 wave by wave (k_symv_trmv's rows) -- one launch less in the hyper-parameter iteration.
template <typename T>
__global__ __launch_bounds__(CHOL_THREADS) void k_safe_symv_trmv(CholBatch<T> bt, SafeSrc<T> src, int64_t ld, int64_t ldx, int64_t lde,
                                                                 int64_t ne, int64_t nt, int32_t* __restrict__ info, int64_t nvalid,
                                                                 unsigned* __restrict__ bar, int32_t* __restrict__ retries,
                                                                 const T* __restrict__ S, const T* __restrict__ X, int64_t ldm,
                                                                 int64_t n, const T* __restrict__ x, T* __restrict__ ys,
                                                                 T* __restrict__ yt) {
  __shared__ __attribute__((aligned(16))) T sm[3 * TILE * LDP];
  __shared__ __attribute__((aligned(16))) T sc[SC_ELEMS];
  __shared__ T piv[TILE];
  (void)chol_safe_body<T>(bt, src, 1, ld, ldx, lde, ne, nt, info, nvalid, bar, retries, sm, sc, piv);
  // (after a fallback its last grid barrier has made X and Sigma visible to every workgroup)
  const int64_t wpb = CHOL_THREADS / 64, nwave = (int64_t)gridDim.x * wpb;
  for (int64_t w = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6); w < 2 * n; w += nwave)
    symv_trmv_row<T>(w, threadIdx.x & 63, S, X, ldm, n, x, ys, yt);
}

// Factorisation by plain launches (matrices beyond the task graph, and the task graph's fallback).  From 8 block columns on it is
// blocked (agp_chol.h, k_chol_panel): groups of G block columns -- the G x G diagonal block by G small launches, the rows below it
// by one panel-solve launch, everything to the right by one trailing launch per group; the part of the trailing update that the
// next group does not need runs on a side stream, next to the next group's diagonal block and panel (look-ahead of one group).
// AGP_CHOL_GROUP = 1 gives the plain per-column right-looking sequence, AGP_CHOL_LOOKAHEAD = 0 keeps everything on one stream.
constexpr int CHOL_GMAX = 8;
static int chol_group() {
  static const int g = []() {
    const char* e = getenv("AGP_CHOL_GROUP");
    const int v = e ? atoi(e) : 8;
    return v < 1 ? 1 : v > CHOL_GMAX ? CHOL_GMAX : v;
  }();
  return g;
}
// blocked from 96 block rows on (extension included): measured on MI355X, a plain 4096 x 4096 matrix (64 block rows) is still
// quicker column by column (2.6 vs 3.0 ms, the group's serial launches dominate), 8192 and the C5 step (64 + 65 rows) are not
static bool chol_blocked(int64_t nt, int64_t ne) { return chol_group() > 1 && nt >= 8 && nt + ne >= 96; }
// kernel launches of one factorisation by plain launches (what the HIP-event timing of the sequence is divided by)
static int64_t chol_launch_count(int64_t nt, int64_t ne) {
  if (!chol_blocked(nt, ne)) return nt;
  const int64_t G = chol_group();
  int64_t n = 0;
  for (int64_t k0 = 0; k0 < nt; k0 += G) {
    const int64_t k1 = (k0 + G < nt) ? k0 + G : nt, kn = (k1 + G < nt) ? k1 + G : nt;
    n += (k1 - k0) + (nt - k1 + ne > 0 ? 1 : 0) + (k1 < nt ? 1 : 0) + (k1 < nt && kn < nt ? 1 : 0);
  }
  return n;
}
static bool chol_lookahead() {
  static const bool on = []() {
    const char* e = getenv("AGP_CHOL_LOOKAHEAD");
    return !(e && e[0] == '0');
  }();
  return on;
}
template <typename T>
static agp_status chol_columns(agp_ctx* c, const CholBatch<T>& bt, int nb, int64_t ld, int64_t ldx, int64_t lde, int64_t ne,
                               int do_x, int64_t nt, int32_t* info_dev, int64_t nvalid) {
  const int64_t G = chol_group();
  if (!chol_blocked(nt, ne)) {
    for (int64_t k = 0; k < nt; ++k) {
      const int64_t nP = nt - k + ne;
      const int64_t nU = chol_nU(k, 0, nt, nt, ne);
      hipLaunchKernelGGL((k_chol_step<T>), dim3((unsigned)(nP + nU), (unsigned)nb), dim3(CHOL_THREADS), 0, c->stream, bt, ld, ldx,
                         lde, ne, do_x, k, nt, info_dev, nvalid, (int64_t)0, (int64_t)-1, (T*)nullptr, (int64_t)0);
    }
    return AGP_OK;
  }
  const int64_t li_stride = G * TILE * TILE;
  const size_t li_need = sizeof(T) * (size_t)(li_stride * nb);
  if (c->chol_li_bytes < li_need) {
    if (c->chol_li) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      (void)hipFree(c->chol_li);
    }
    c->chol_li = nullptr;
    c->chol_li_bytes = 0;
    if (hipMalloc(&c->chol_li, li_need) != hipSuccess) return AGP_ERR_NOMEM;
    c->chol_li_bytes = li_need;
  }
  T* li = (T*)c->chol_li;
  const bool look = chol_lookahead();
  if (look && !c->side) {
    HIPCHK(c, hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
  }
  auto trail = [&](hipStream_t st, int64_t k0, int64_t k1, int64_t j_lo, int64_t j_hi) {
    const int64_t n = chol_trail_tiles(j_lo, j_hi, nt, ne);
    if (n > 0)
      hipLaunchKernelGGL((k_chol_trail<T>), dim3((unsigned)n, (unsigned)nb), dim3(CHOL_THREADS), 0, st, bt, ld, lde, ne, k0, k1,
                         nt, j_lo, j_hi);
  };
  bool side_busy = false;
  for (int64_t k0 = 0; k0 < nt; k0 += G) {
    const int64_t k1 = (k0 + G < nt) ? k0 + G : nt;
    const int g = (int)(k1 - k0);
    // D: the diagonal block on its own (block rows k0 .. k1-1 only), leaving the inverses of its diagonal tiles in li
    for (int64_t k = k0; k < k1; ++k) {
      const int64_t nP = k1 - k;
      const int64_t nU = chol_nU(k, k0, k1, k1, 0);
      hipLaunchKernelGGL((k_chol_step<T>), dim3((unsigned)(nP + nU), (unsigned)nb), dim3(CHOL_THREADS), 0, c->stream, bt, ld, ldx,
                         lde, (int64_t)0, do_x, k, k1, info_dev, nvalid, k0, k1, li, li_stride);
    }
    // P: block rows k1 .. nt-1 and the extension rows against the block
    const int64_t rows = nt - k1 + ne;
    if (rows > 0) {
      const dim3 grid((unsigned)rows, (unsigned)nb);
#define AGP_PANEL(GG)                                                                                                       \
  hipLaunchKernelGGL((k_chol_panel<T, GG>), grid, dim3(CHOL_THREADS), 0, c->stream, bt, ld, lde, ne, k0, nt, (const T*)li, \
                     li_stride, g)
      if (G <= 2) AGP_PANEL(2);
      else if (G <= 4) AGP_PANEL(4);
      else AGP_PANEL(8);
#undef AGP_PANEL
    }
    if (k1 >= nt) break;
    // T: the far columns were last written by the previous group's side-stream launch: order behind it
    if (side_busy) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
    const int64_t kn = (k1 + G < nt) ? k1 + G : nt;  // the next group's columns [k1, kn) are needed first
    trail(c->stream, k0, k1, k1, kn);
    if (kn < nt) {
      if (look) {
        HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
        trail(c->side, k0, k1, kn, nt);
        HIPCHK(c, hipEventRecord(c->ev_join, c->side));
        side_busy = true;
      } else {
        trail(c->stream, k0, k1, kn, nt);
      }
    }
  }
  if (side_busy) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
  return AGP_OK;
}

static void dag_pause(agp_ctx* c) {
  c->dag_off = true;
  c->dag_cooldown = c->dag_backoff;
  c->dag_backoff = std::min<int64_t>(c->dag_backoff * 4, (int64_t)1 << 20);
}
// once per CAVI step: end of the probation?
static void dag_tick(agp_ctx* c) {
  if (c->dag_off && --c->dag_cooldown <= 0) c->dag_off = false;
}
// host side of the latch: called where the stream has just been synchronised anyway
static void dag_retry_check(agp_ctx* c) {
  if (!c->safe_retries || c->dag_off) return;
  int32_t r = 0;
  if (hipMemcpy(&r, c->safe_retries, sizeof(r), hipMemcpyDeviceToHost) != hipSuccess) return;
  if (r > c->dag_retries_seen) {
    fprintf(stderr,
            "[agp_hip] warning: %d task-graph factorisation(s) lost a tile dependency (is another process using this GPU?) and were "
            "re-run by the in-stream fallback; this context uses plain launches for the next %lld steps\n",
            (int)(r - c->dag_retries_seen), (long long)c->dag_backoff);
    c->dag_retries_seen = r;
    dag_pause(c);
  }
}

// Split task-graph launches: worth it when the launch queues far more tiles than the chip has workgroup slots (C3: 1584, C4: 3264);
// the small launches (C2: 408 tiles, and its merged step with the prologue) stay one kernel.  AGP_CHAIN_SPLIT=0 / 1 forces.
static bool chain_split_wanted(int64_t tiles, bool with_prologue = false, bool f64 = true) {
  static const int v = []() {
    const char* e = getenv("AGP_CHAIN_SPLIT");
    return e ? (e[0] == '0' ? 0 : 1) : -1;
  }();
  // fp64 launches with the prologue stay merged unless forced: their tile workgroups stage four LDS tiles (135 KB: one workgroup
  // per CU whatever the registers), and the measured case lost (C2: 0.3167 ms split, 0.3103 ms merged).  In fp32 the same tile
  // kernel fits two workgroups per CU (68 KB, 128 VGPRs) and wins: m = 1024, B = 2048 fp32 0.325 -> 0.270 ms per step.
  // Round 5 made the fp32 form opt-in as well after two findings of the stress runs (docs/DESIGN_LOG.md section 14): the chain kernel
  // took tile (0, 0)'s eta2 step, so an ABORTED launch could leave eta2 half-stepped (repaired in round 5: the chain's place in the
  // tile kernel takes it and parks the tile), and about one split launch in 10 000 lost a dependency on its own -- the tile kernel
  // filled every CU before the chain kernel was resident (repaired in round 6: DagSync::here / k_wait_here).  Default again in fp32.
  if (with_prologue && f64 && v < 0) return false;
  return v < 0 ? tiles >= 600 : v == 1;
}
// the chain stream, its release word and the proof that kernels of the two streams run at the same time (k_handshake: where
// dispatches are serialised -- rocprofv3 --pmc, AMD_SERIALIZE_KERNEL -- a chain kernel polling for the tile kernel behind it in
// the device's single queue would never be released; such a context keeps the merged kernel)
static bool chain_split_ready(agp_ctx* c) {
  if (c->chain_state != 0) return c->chain_state == 1;
  c->chain_state = -1;
  int lo = 0, hi = 0;
  if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) return false;
  if (hipStreamCreateWithPriority(&c->chain_stream, hipStreamNonBlocking, hi) != hipSuccess) {
    c->chain_stream = nullptr;
    (void)hipGetLastError();
    return false;
  }
  bool ok = hipExtMallocWithFlags((void**)&c->chain_go, 8, hipMallocSignalMemory) == hipSuccess && hipMemset(c->chain_go, 0, 8) == hipSuccess &&
            hipMalloc((void**)&c->chain_ctr, sizeof(int32_t)) == hipSuccess && hipMemset(c->chain_ctr, 0, sizeof(int32_t)) == hipSuccess;
  int32_t* hs = nullptr;
  ok = ok && hipMalloc((void**)&hs, 4 * sizeof(int32_t)) == hipSuccess && hipMemset(hs, 0, 4 * sizeof(int32_t)) == hipSuccess;
  if (ok) {
    (void)hipStreamSynchronize(c->stream);
    hipLaunchKernelGGL(k_handshake, dim3(1), dim3(64), 0, c->chain_stream, hs, (const int32_t*)(hs + 1), hs + 2);
    hipLaunchKernelGGL(k_handshake, dim3(1), dim3(64), 0, c->stream, hs + 1, (const int32_t*)hs, hs + 3);
    int32_t res[4] = {0, 0, 0, 0};
    ok = hipStreamSynchronize(c->chain_stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess &&
         hipMemcpy(res, hs, sizeof(res), hipMemcpyDeviceToHost) == hipSuccess && res[2] == 1 && res[3] == 1;
  }
  if (hs) (void)hipFree(hs);
  (void)hipGetLastError();
  if (ok) c->chain_state = 1;
  return ok;
}
// Behind a split launch NO event joins the two streams: the tile kernel cannot end before the chain's last publish, after which the
// chain writes nothing (an fp64 step launch stores no diagonal factors, dag_store_dg in agp_chol.h; an fp32 one issues them as
// write-through stores before that publish), so whatever follows on this
// context's stream -- and a host synchronisation of it -- sees a finished factorisation.  The one exception, an aborted launch whose
// chain is still inside a tile factorisation, is handled where it matters: the fallback waits for the chain workgroups' exit count
// (DagSync::done, SafeSrc::chain_done).  (An event join -- record on the chain stream, wait on this one -- was the first version and
// DEADLOCKED with the host several steps ahead, the look-ahead on and the prologue inside the split launch; removed in round 5,
// the account is in docs/DESIGN_LOG.md.)
// what a split launch hands its kernels / its fallback about the chain kernel (nb chain workgroups)
static void chain_split_arm(agp_ctx* c, DagSync& ds, int nb) {
  ds.go = c->chain_go;
  ds.go_val = ++c->chain_seq;
  ds.done = c->chain_ctr;
  ds.here = c->chain_go + 1;  // (second word of the same signal-memory allocation)
  c->chain_exits += nb;
}
// ... enqueued on the step's stream between the chain kernel's launch (chain stream) and the tile kernel's: every chain workgroup
// of this launch -- and of all launches before it: the count is cumulative, like chain_exits -- is resident (DagSync::here)
static void chain_split_wait_here(agp_ctx* c) {
  hipLaunchKernelGGL(k_wait_here, dim3(1), dim3(64), 0, c->stream, (const int32_t*)(c->chain_go + 1), c->chain_exits);
}

// what a CAVI step hands to its factorisation about the look-ahead stream (see DagSync, agp_chol.h)
struct StepSync {
  DagSync ds{};
  bool used = false;  // out: the task-graph launch took `ds`
};

// k-slices per block column of the prologue's product S = kappa' diag(w) kappa: ks[c] for the tiles of block column c, kf[c] for its
// PRO_NEAR tiles next to the diagonal (the chain's feeders).  Columns 0 and 1 feed the chain at once and are split as far as it
// pays.  pre: the chain's first tiles were prepared by the launch in front (ProArgs::pre), so it reaches every column ~10 us sooner.
// Two fits:
//  * fp32, and fp64 up to three block columns -- the first fit, kept as it is (fp32 was not measured again; at two and three block
//    columns the bit-pinned tests run): a tile of column c has tau c - head for its product, tau = 17.8 / 14 us the chain's pace then,
//    a 64-row chunk costing tc + 0.3 = 3.0 / 1.9 us; near tiles split like their column.
//  * fp64 from four block columns on -- fitted to the stamps of the C2 launch (16 columns, nq = 16; tools/step_boundary.py, DESIGN.md
//    section 5).  The tile that came late was the DIAGONAL feeder (c, c): the look under factor(c - 1) wants it parked, and before
//    that it forms its slice of the product (tc per chunk), takes the eta2 step (te) and applies the updates of columns 0 .. c - 2
//    (tu each), the last of which arrives tl behind factor(c - 2).  Its workgroup starts ts0 + ts1 c after the launch's first one
//    (the columns in front hold the slots).  With the chain at tau per column and factor(0) done f0 after the start:
//        chunks tc <= f0 + tau (c - 2) + tl - margin - te - tu (c - 2) - (ts0 + ts1 c)  =  (tau - tu - ts1) c - head_near
//    The other tiles of the column have to be ready when X_c is out: one column later, one update more.  In column 0 only the near
//    tiles are urgent; the others give half of their helpers away (112 -> 64 workgroups in front of everything else: tile (2, 2)
//    started 12 us into the launch).
static void pro_ks_table(int64_t nt, int64_t nq, bool f64, unsigned char* ks, unsigned char* kf, bool pre = false) {
  const int cap = (int)std::min<int64_t>(8, nq);
  auto split = [&](double work, double budget) { return std::max(1, std::min(cap, (int)std::ceil(work / std::max(budget, 1.0)))); };
  if (nt <= 3 || !f64) {
    const double tc = f64 ? 2.7 : 1.6, tau = f64 ? 17.8 : 14.0, head = pre ? 24.0 : 12.0;
    for (int64_t c = 0; c < nt && c < 32; ++c)
      ks[c] = kf[c] = (unsigned char)(c == 0 ? cap : c == 1 ? std::min(cap, f64 ? 4 : 8) : split((double)nq * (tc + 0.3), tau * (double)c - head));
    return;
  }
  // us, measured: tc 3.05 - 3.2 on single tiles (3.4 taken: with 3.1 tile (7, 7) kept its whole product, and the looks under
  // factor(6) and factor(7) failed in 8 - 10 % of the launches), tau 16.2, f0 17.4 with the prepared head
  const double tc = 3.4, tau = 16.2, tu = 4.0, te = 4.0, tl = 6.0, ts0 = 7.0, ts1 = 2.5, margin = 3.0, f0 = pre ? 17.4 : 27.4;
  const double slope = tau - tu - ts1;                                             // 9.7
  const double head_near = 2.0 * tau - 2.0 * tu + ts0 + te + margin - tl - f0;     // 15.0 with pre
  const double head_far = head_near - (tau + tl - tu - margin);                    // -0.2
  kf[0] = (unsigned char)cap, ks[0] = (unsigned char)std::min(cap, 4);
  kf[1] = ks[1] = (unsigned char)std::min(cap, 4);
  for (int64_t c = 2; c < nt && c < 32; ++c) {
    kf[c] = (unsigned char)split((double)nq * tc, slope * (double)c - head_near);
    ks[c] = (unsigned char)split((double)nq * tc, slope * (double)c - head_far);
  }
}
// test hook (AGP_DAG_TEST_ABORT=1): pretend every task-graph launch of a CAVI step lost a dependency, so that the in-stream
// fallback runs behind each of them
static bool dag_test_abort() {
  static const bool on = []() {
    const char* e = getenv("AGP_DAG_TEST_ABORT");
    return e && e[0] == '1';
  }();
  return on;
}

// test hook (AGP_DAG_TEST_FEED=1 / 2): how the chain's side job treats the two feeder tiles of the next block column (ChainPrefetch,
// agp_chol.h) -- 1: every prefetched D element counts as not yet visible and is settled again ; 2: every look reports "not parked",
// so every column takes the blocking fetch.  Both re-load valid data: results are bit for bit those of the default path.
static int dag_test_feed() {
  static const int v = []() {
    const char* e = getenv("AGP_DAG_TEST_FEED");
    return e && e[0] == '1' ? 1 : e && e[0] == '2' ? 2 : 0;
  }();
  return v;
}

// ---- the task-graph launch (k_chol_dag) -------------------------------------------------------------------------------
// the flag array of the task graph: at least nf epoch-stamped words (grown with some slack; a new array starts at epoch 0)
static agp_status dag_flags_ensure(agp_ctx* c, int64_t nf) {
  if (c->dag_cap < nf) {
    if (c->dag_flags) (void)hipFree(c->dag_flags);
    c->dag_flags = nullptr;
    c->dag_cap = 0;
    if (hipMalloc((void**)&c->dag_flags, sizeof(int32_t) * (size_t)(nf + 1024)) != hipSuccess) return AGP_ERR_NOMEM;
    c->dag_cap = nf + 1024;
    HIPCHK(c, hipMemsetAsync(c->dag_flags, 0, sizeof(int32_t) * (size_t)c->dag_cap, c->stream));
    c->dag_epoch = 0;
  }
  return AGP_OK;
}
// The pending refill of hand-over set `other` (left dirty by a single-problem launch of the same element type) is taken over by the
// launch being prepared: its trailing (ProArgs::fill) or product (ProdArgs::fill) workgroups store the sentinels in its shadow.
// false: nothing to take
template <typename T>
static bool dag_take_refill(agp_ctx* c, int other, T** fill, int64_t* fill_n) {
  auto& d = c->h_dirty[other];
  if (!(c->hset[other] && d.on && d.nb == 1 && c->htype == (int)sizeof(T))) return false;
  *fill = (T*)c->hset[other];
  *fill_n = d.used;
  d.on = false;
  return true;
}

// The instantiations of k_chol_dag the driver launches, by name (always FUSED, never TRACE; ROLE belongs to dag_launch).  STEP also
// is the launch-uniform choice of the slot format without X21 and of the block substitution (dag_block_subst, agp_chol.h): every
// kernel of a launch, merged or split, is instantiated with the same T / STEP / BATCH and so reads the same decision.
template <bool BATCH_, bool STEP_, bool PRO_>
struct DagKernel { static constexpr bool BATCH = BATCH_, STEP = STEP_, PRO = PRO_; };
using DagFactor = DagKernel<false, false, false>;    // a factor with whatever rides along: L, its inverse, P = X' X
using DagFactorPro = DagKernel<false, false, true>;  // ... behind the pending natural-gradient step (hyper-parameter iteration)
using DagStep = DagKernel<false, true, false>;       // the CAVI step's launch (extension rows only): specialised, may go out split
using DagStepPro = DagKernel<false, true, true>;     // ... with the pending step as its prologue (and the rows as its epilogue)
using DagStepBatch = DagKernel<true, true, false>;   // the CAVI step's launch for nb interleaved problems

// what a launch hands to k_chol_dag next to the context's flag array and epoch -- the same to both kernels of a split launch
template <typename T>
struct DagArgs {
  CholBatch<T> bt{};
  int nb = 1;
  int64_t fstride = 0, ld = 0, ldx = 0, lde = 0, ne = 0, nt = 0;
  int32_t* info = nullptr;
  int64_t nvalid = 0;
  unsigned long long* trace = nullptr;  // (wall-clock stamps of the prologue and the step boundary, PRO_TS / STRACE in agp_chol.h)
  T* H = nullptr;
  int64_t hstride = 0, nx = 0;
  const T* erow = nullptr;
  int opts = 0;
  DagSync ds{};
  ProArgs<T> pro{};  // (a launch without the rider passes the default)
  EpiArgs<T> epi{};
  ProdArgs<T> prod{};
};
template <typename T, typename K, int ROLE>
static void dag_enqueue(agp_ctx* c, unsigned grid, hipStream_t stream, const DagArgs<T>& a) {
  hipLaunchKernelGGL((k_chol_dag<T, true, K::BATCH, false, K::STEP, K::PRO, ROLE>), dim3(grid), dim3(CHOL_THREADS), 0, stream, a.bt,
                     a.nb, a.fstride, a.ld, a.ldx, a.lde, a.ne, a.nt, a.info, a.nvalid, c->dag_flags, c->dag_epoch, a.trace, a.H,
                     a.hstride, a.nx, a.erow, a.opts | (dag_test_feed() << 2), a.ds, a.pro, a.epi, a.prod);
}
// One task-graph launch of `grid` workgroups on the context's stream -- or, split (STEP instantiations only), as two kernels: the
// a.nb chain workgroups on their own stream (enqueued first), every other tile on this one, behind the wait for the chains' residency
template <typename T, typename K>
static agp_status dag_launch(agp_ctx* c, unsigned grid, bool split, DagArgs<T>& a) {
  if constexpr (K::STEP) {
    if (split) {
      chain_split_arm(c, a.ds, a.nb);
      dag_enqueue<T, K, 1>(c, (unsigned)a.nb, c->chain_stream, a);
      chain_split_wait_here(c);
      dag_enqueue<T, K, 2>(c, grid, c->stream, a);
      LAUNCHCHK(c);
      return AGP_OK;
    }
  }
  dag_enqueue<T, K, 0>(c, grid, c->stream, a);
  LAUNCHCHK(c);
  return AGP_OK;
}

// What potrf_fused is asked for: Cholesky (lower, in place; diagonal factors in Dg) of the n x n matrix A (n = nt * 64) with `ne`
// extension row blocks E <- E L^-T; X takes the inverses of the diagonal tiles, with do_x all of L^-1.  The riders are optional.
template <typename T>
struct PotrfReq {
  T *A = nullptr, *X = nullptr, *Dg = nullptr, *E = nullptr;
  int64_t ld = 0, n = 0, ldx = 0, lde = 0, ne = 0;
  int do_x = 0;
  int32_t* info_dev = nullptr;  // failures latch here; rows from nvalid on are padding
  int64_t nvalid = 0;
  // erow: the last extension block is [erow' ; 0] (not yet written to E: the task graph reads it in place; the per-column
  // path needs it in E first)
  const T* erow = nullptr;
  // want_l = false: the caller never reads the factor L itself (only E L^-T, X, Dg): the task graph skips those stores
  bool want_l = true;
  // safe: sources the inputs can be restored from (A = -2 eta2, E = [kappa ; eta1' ; 0]): the in-stream fallback k_chol_safe is
  // then enqueued behind the task graph; without it a lost dependency surfaces as an error at the caller's next check
  SafeSrc<T>* safe = nullptr;
  // defer_safe (in: the caller can run the fallback itself, k_safe_rowstats; out: whether it has to -- the task graph was used)
  bool defer_safe = false;
  // ssync (CAVI step next to a look-ahead stream): the step's task-graph instantiation stores its `started` number (`used` is set)
  StepSync* ssync = nullptr;
  // pro: the pending natural-gradient step that the launch takes along as its prologue (ProArgs, agp_chol.h).  The caller fills
  // the step's own fields; the driver sets what it owns: HS, sflags, fill, fill_n, nfill, ks, kf
  const ProArgs<T>* pro = nullptr;
  const EpiArgs<T>* epi = nullptr;  // (with pro, on the CAVI step's launch) the row statistics as the launch's epilogue
  // Pout (with do_x; leading dimension ldx): P = X' X is wanted next -- K^-1 at a kernel refresh, Sigma for the hyper-gradient.  On
  // the task graph it is formed by product workgroups at the end of the same launch (ProdArgs, agp_chol.h) and p_done (out) says
  // so; otherwise the caller forms it (xtx_padded).  ld_out / ld_status: ProdArgs::ld_out / status
  T* Pout = nullptr;
  bool p_done = false;
  double* ld_out = nullptr;
  int32_t* ld_status = nullptr;
};

template <typename T>
static agp_status potrf_fused(agp_ctx* c, PotrfReq<T>& r) {
  r.p_done = false;
  const bool can_defer = r.defer_safe;
  r.defer_safe = false;
  const int64_t nt = r.n / TILE, ne = r.ne;
  const bool use_dag = chol_use_dag(c, nt, ne);
  if (r.pro && !(use_dag && r.X && !r.want_l && nt <= 32)) {
    c->err = "potrf_fused: a pending natural-gradient step can only ride on the CAVI step's task-graph launch";
    return AGP_ERR_INVALID;
  }
  CholBatch<T> one{};
  one.A[0] = r.A, one.X[0] = r.X, one.Dg[0] = r.Dg, one.E[0] = r.E;
  if (use_dag && r.X) {
    const int64_t nx = (r.do_x && nt > 1) ? nt : 0;  // the full inverse rides along as nt identity block rows
    DagArgs<T> a{};
    // prologue (pro): helper workgroups, their flags and hand-over slots
    ProArgs<T>& pa = a.pro;
    int64_t nhelp = 0;
    if (r.pro) {
      pa = *r.pro;
      if (pa.packed)
        for (int64_t cc = 0; cc < nt; ++cc) pa.ks[cc] = pa.kf[cc] = 1;  // nothing to compute: no helpers
      else
        pro_ks_table(nt, pa.Kdim / TILE, sizeof(T) == 8, pa.ks, pa.kf, pa.pre != nullptr);
      for (int64_t cc = 0; cc < nt; ++cc) nhelp += pro_nhelp(nt, cc, pa.ks[cc], pa.kf[cc]);
    }
    AGPCHK(dag_flags_ensure(c, ((nt + ne + nx) * nt + 3 * nt + 1 + nhelp) * DAG_FS));
    c->dag_epoch += 1;
    const int64_t ntiles = nt * (nt + 1) / 2 + ne * nt + (nx ? nt * (nt + 1) / 2 : 0);
    const int64_t hstride = ((2 * nt + ne) * nt + 3 * nt + nhelp) * TILE * TILE;
    const int64_t hused = (3 * nt + (nt + ne + nx) * nt + nhelp) * TILE * TILE;
    const bool with_p = r.Pout != nullptr && nx > 0;
    const int64_t nprod = with_p ? nt * (nt + 1) / 2 : 0;
    // launches with a prologue alternate between the two hand-over sets and refill each other's; so do the launches with product
    // workgroups (the symmetric-product launches whose riders refilled set 0 behind them are gone from their path)
    const int hs = (r.pro || with_p) ? c->h_step_set : 0;
    AGPCHK(dag_handover_acquire<T>(c, hstride, hs, &a.H));
    ProdArgs<T>& pd = a.prod;
    if (with_p) {
      pd.out = r.Pout, pd.ld = r.ldx;
      pd.ld_out = r.ld_out, pd.status = r.ld_status;  // (log det of the factor rides on the last product workgroup)
      if (!r.pro) {
        (void)dag_take_refill<T>(c, hs ^ 1, &pd.fill, &pd.fill_n);
        c->h_step_set = hs ^ 1;
      }
      if (r.safe) {
        r.safe->pout = r.Pout, r.safe->ldpo = r.ldx;
        r.safe->ld_out = r.ld_out, r.safe->ld_status = r.ld_status, r.safe->ld_n = r.nvalid;
      }
      r.p_done = true;
    }
    // the CAVI step's launch (DagStep / DagStepPro); everything else is a DagFactor / DagFactorPro
    const bool step_inst = nx == 0 && !r.do_x && !r.want_l;
    if (r.ssync && step_inst) a.ds = r.ssync->ds, r.ssync->used = true;
    a.bt = one, a.ld = r.ld, a.ldx = r.ldx, a.lde = r.lde, a.ne = ne, a.nt = nt, a.info = r.info_dev, a.nvalid = r.nvalid;
    a.hstride = hstride, a.nx = nx, a.erow = r.erow, a.opts = (int)(r.do_x && nx == 0) | (r.want_l ? 2 : 0);
    if (r.pro) {  // ... with the pending natural-gradient step as its prologue (the CAVI step's launch, or --
                  // hyper-parameter iteration -- the factorisation of the updated -2 eta2 with its inverse)
      pa.HS = a.H + (3 * nt + (nt + ne + nx) * nt) * TILE * TILE;
      pa.sflags = c->dag_flags + ((nt + ne + nx) * nt + 3 * nt + 1) * DAG_FS;
      // the set the launch before this one used: refilled in this launch's shadow
      if (dag_take_refill<T>(c, hs ^ 1, &pa.fill, &pa.fill_n)) pa.nfill = 64;
      a.trace = step_inst ? step_trace_next(c) : nullptr;
      c->strace_last = a.trace;
      if (step_inst && r.epi) a.epi = *r.epi;
    }
    const int64_t base = ntiles + nhelp + pa.nfill;  // tile, helper and refill workgroups; the product workgroups come last
    if (!step_inst) pd.base = base;
    // chain kernel + tile kernel (k_chol_dag, ROLE)?
    const bool split = step_inst && chain_split_wanted(ntiles + nhelp, r.pro != nullptr, sizeof(T) == 8) && chain_split_ready(c);
    // No event joins the chain stream behind a split launch (see chain_split_arm): correct only as long as the chain kernel
    // stores nothing after its last publish.  C = S + K^-1 / 4 (ProArgs::Cout) is a plain store of tile (0, 0)'s workgroup --
    // in a split launch that would be the chain kernel, whose plain stores only become visible when THAT kernel ends.  Cout
    // exists for launches with the inverse (do_x), which never split; enforced here rather than assumed.
    if (split && pa.Cout) {
      c->err = "potrf_fused: C = S + K^-1/4 (ProArgs::Cout) cannot ride on a split (chain kernel + tile kernel) launch";
      return AGP_ERR_INVALID;
    }
    const unsigned grid = (unsigned)(base + nprod);
    if (r.pro)
      AGPCHK(step_inst ? (dag_launch<T, DagStepPro>(c, grid, split, a)) : (dag_launch<T, DagFactorPro>(c, grid, split, a)));
    else
      AGPCHK(step_inst ? (dag_launch<T, DagStep>(c, grid, split, a)) : (dag_launch<T, DagFactor>(c, grid, split, a)));
    if (r.pro) c->h_step_set = hs ^ 1;
    AGPCHK(dag_handover_release<T>(c, hused, hstride, 1, hs));
    if (r.safe) {  // (a split launch's fallback waits for the chain's exit count)
      r.safe->chain_done = split ? c->chain_ctr : nullptr;
      r.safe->chain_want = c->chain_exits;
    }
    if (r.safe && (!r.do_x || r.safe->want_x)) {
      if (dag_test_abort()) hipLaunchKernelGGL(k_set_i32, dim3(1), dim3(1), 0, c->stream, r.info_dev, -1);
      if (can_defer) r.defer_safe = true;
      else AGPCHK(launch_chol_safe<T>(c, one, *r.safe, 1, r.ld, r.ldx, r.lde, ne, nt, r.info_dev, r.nvalid));
    }
    return AGP_OK;  // X = L^-1 came out of the same launch
  }
  if (r.erow && ne > 0)
    hipLaunchKernelGGL((k_set_ext_rows<T>), dim3((unsigned)((TILE * r.n + 255) / 256)), dim3(256), 0, c->stream,
                       r.E + (ne - 1) * TILE * r.lde, r.lde, r.n, r.erow);
  AGPCHK(chol_columns<T>(c, one, 1, r.ld, r.ldx, r.lde, ne, r.do_x, nt, r.info_dev, r.nvalid));
  LAUNCHCHK(c);
  if (r.do_x) AGPCHK(trtri_levels<T>(c, (const T*)r.A, r.ld, r.X, r.ldx, nt));
  return AGP_OK;
}

// Task-graph launches whose inputs cannot be restored on the device (the factor is written in place: K_ZZ, the building blocks;
// or the inverse rides along) are checked on the host instead: synchronise, and if the latch reads -1 stop using the task graph
// on this context and tell the caller to rebuild its input and factor again (now with per-column launches).
static agp_status dag_lost_dependency(agp_ctx* c, int32_t* info_dev, bool* lost) {
  *lost = false;
  int32_t info = 0;
  HIPCHK(c, hipMemcpyAsync(&info, info_dev, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (info == -1) {
    HIPCHK(c, hipMemsetAsync(info_dev, 0, sizeof(int32_t), c->stream));
    if (!c->dag_off)
      fprintf(stderr, "[agp_hip] warning: a task-graph factorisation lost a tile dependency (is another process using this GPU?); "
                      "re-running it with plain launches, which this context uses for the next %lld steps\n",
              (long long)c->dag_backoff);
    dag_pause(c);
    *lost = true;
  }
  return AGP_OK;
}

// nb independent problems of identical shape (bt; no X = L^-1): what potrf_dag_batch / potrf_fused_batch are asked for
template <typename T>
struct PotrfBatchReq {
  const CholBatch<T>* bt = nullptr;
  int nb = 0;
  int64_t ld = 0, n = 0, ldx = 0, lde = 0, ne = 0;
  int32_t* info_dev = nullptr;
  int64_t nvalid = 0;
  SafeSrc<T>* safe = nullptr;  // (task graph) as in PotrfReq
};

// nb <= DAG_MAX_NB independent problems of identical shape as ONE interleaved task-graph launch (see k_chol_dag): their chains
// run side by side on nb CUs (workgroup index = tile * nb + problem: with 8 problems each one lives on its own XCD).
constexpr int DAG_MAX_NB = 8;
template <typename T>
static agp_status potrf_dag_batch(agp_ctx* c, const PotrfBatchReq<T>& r) {
  const int nb = r.nb;
  const int64_t nt = r.n / TILE, ne = r.ne;
  const int64_t fstride = ((nt + ne) * nt + 3 * nt + 1) * DAG_FS;
  AGPCHK(dag_flags_ensure(c, fstride * nb));
  c->dag_epoch += 1;
  const int64_t ntiles = nt * (nt + 1) / 2 + ne * nt;
  const int64_t hstride = ((2 * nt + ne) * nt + 3 * nt) * TILE * TILE;
  const int hs = 0;
  DagArgs<T> a{};
  AGPCHK(dag_handover_acquire<T>(c, hstride * nb, hs, &a.H));
  a.bt = *r.bt, a.nb = nb, a.fstride = fstride, a.ld = r.ld, a.ldx = r.ldx, a.lde = r.lde, a.ne = ne, a.nt = nt;
  a.info = r.info_dev, a.nvalid = r.nvalid, a.hstride = hstride;
  // the nb chains as one kernel, all other tiles as another?
  const bool split = chain_split_wanted(ntiles * nb) && chain_split_ready(c);
  AGPCHK((dag_launch<T, DagStepBatch>(c, (unsigned)(ntiles * nb), split, a)));
  AGPCHK(dag_handover_release<T>(c, (3 * nt + (nt + ne) * nt) * TILE * TILE, hstride, nb, hs));
  if (r.safe) {
    r.safe->chain_done = split ? c->chain_ctr : nullptr;
    r.safe->chain_want = c->chain_exits;
    if (dag_test_abort()) hipLaunchKernelGGL(k_set_i32, dim3(1), dim3(1), 0, c->stream, r.info_dev, -1);
    AGPCHK(launch_chol_safe<T>(c, *r.bt, *r.safe, nb, r.ld, r.ldx, r.lde, ne, nt, r.info_dev, r.nvalid));
  }
  return AGP_OK;
}

// the same factorisation for nb <= CHOL_MAXB independent problems of identical shape in shared launches (no X = L^-1)
template <typename T>
static agp_status potrf_fused_batch(agp_ctx* c, const PotrfBatchReq<T>& r) {
  AGPCHK(chol_columns<T>(c, *r.bt, r.nb, r.ld, r.ldx, r.lde, r.ne, 0, r.n / TILE, r.info_dev, r.nvalid));
  LAUNCHCHK(c);
  return AGP_OK;
}
