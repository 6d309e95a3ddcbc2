// agp_comm_host.h -- host side of the collectives (struct agp_comm and the RCCL loader: agp_comm.h): one sum through whichever
// transport the communicator has (comm_issue), its event timing, the train of ranges on the communicator's own stream
// (comm_allreduce_groups, called by Svgp<T>'s multi-GPU step in agp_capi.hip) and the diagnostic stand-in for a ring all-reduce
// (k_standin_allreduce, the one kernel of this header).  The agp_comm_* entry points are in agp_capi.hip.
#pragma once
#include <string>

#include "agp_chol.h"
#include "agp_chol_host.h"  // k_set_arrive
#include "agp_comm.h"
#include "agp_ctx.h"

// one in-place sum on `stream` through whichever transport the communicator has
static agp_status comm_issue(agp_comm* cm, void* buf, int64_t count, int32_t dtype, hipStream_t stream) {
  agp_ctx* ctx = cm->ctx;
  if (cm->kind == 0) {
    std::string why;
    RcclApi* api = rccl_api(why);
    if (!api) return AGP_ERR_UNSUPPORTED;
    ncclResult_t r = api->AllReduce(buf, buf, (size_t)count, dtype == AGP_F64 ? ncclFloat64 : ncclFloat32, ncclSum, cm->nccl, stream);
    if (r != ncclSuccess) {
      ctx->err = std::string("ncclAllReduce : ") + api->GetErrorString(r);
      return AGP_ERR_HIP;
    }
  } else {
    const int32_t r = cm->fn(cm->user, buf, count, dtype, (void*)stream);
    if (r != 0) {
      ctx->err = "agp_comm: the host all-reduce callback failed with code " + std::to_string(r);
      return AGP_ERR_HIP;
    }
  }
  return AGP_OK;
}
static agp_status comm_timing_begin(agp_comm* cm, hipStream_t stream) {
  agp_ctx* ctx = cm->ctx;
  cm->timing_now = cm->timing && ((cm->n_calls - 1) % cm->timing_every == 0);
  if (cm->timing_now) {
    if (cm->ev_used + 2 > cm->ev.size())
      for (int i = 0; i < 2; ++i) {
        hipEvent_t e;
        HIPCHK(ctx, hipEventCreate(&e));
        cm->ev.push_back(e);
      }
    HIPCHK(ctx, hipEventRecord(cm->ev[cm->ev_used], stream));
  }
  return AGP_OK;
}
static agp_status comm_timing_end(agp_comm* cm, hipStream_t stream) {
  agp_ctx* ctx = cm->ctx;
  if (cm->timing_now) {
    HIPCHK(ctx, hipEventRecord(cm->ev[cm->ev_used + 1], stream));
    cm->ev_used += 2;
    cm->n_timed += 1;
  }
  return AGP_OK;
}

// AGP_SPLIT_OVERLAP: the batch-parallel statistics as a train of `ng` ranges (block-column groups, agp_chol.h pack_index) on the
// communicator's OWN stream, ordered after what the ctx's stream holds now; after range g a one-thread kernel stores `epoch` into
// arrive[g * ARRIVE_STRIDE], which the tile workgroups of the NEXT task-graph launch poll (pro_arrival_gate) -- that launch is
// enqueued on the ctx's stream right away and starts on group 0 while the others are still travelling.  Nothing on the ctx's stream
// waits for the train (cm->ev_out is there for a flush that wants the whole statistic).  Counted as ONE collective call of the sum
// of the ranges for agp_comm_stats; with timing on, the events bracket the whole train on the side stream.
static agp_status comm_allreduce_groups(agp_comm* cm, void* base, int esz, const int64_t* off, const int64_t* cnt, int ng,
                                        int32_t dtype, int32_t* arrive, int32_t epoch) {
  agp_ctx* ctx = cm->ctx;
  DevGuard guard(ctx->device);
  if (!cm->side) {
    int lo = 0, hi = 0;
    HIPCHK(ctx, hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIPCHK(ctx, hipStreamCreateWithPriority(&cm->side, hipStreamNonBlocking, hi));
    HIPCHK(ctx, hipEventCreateWithFlags(&cm->ev_in, hipEventDisableTiming));
    HIPCHK(ctx, hipEventCreateWithFlags(&cm->ev_out, hipEventDisableTiming));
  }
  HIPCHK(ctx, hipEventRecord(cm->ev_in, ctx->stream));
  HIPCHK(ctx, hipStreamWaitEvent(cm->side, cm->ev_in, 0));
  cm->n_calls += 1;
  AGPCHK(comm_timing_begin(cm, cm->side));
  for (int g = 0; g < ng; ++g) {
    cm->bytes += cnt[g] * esz;
    AGPCHK(comm_issue(cm, (char*)base + off[g] * esz, cnt[g], dtype, cm->side));
    hipLaunchKernelGGL(k_set_arrive, dim3(1), dim3(1), 0, cm->side, arrive + g * ARRIVE_STRIDE, epoch);
    LAUNCHCHK(ctx);
  }
  AGPCHK(comm_timing_end(cm, cm->side));
  HIPCHK(ctx, hipEventRecord(cm->ev_out, cm->side));
  return AGP_OK;
}

// ---- stand-in for an xGMI ring all-reduce on a one-GPU box (diagnostic; agp_comm_standin_allreduce) -------------------------------
// RCCL's ring kernel is a handful of workgroups ("channels") that pass chunks to one another through flags: it only finishes when all
// of them are RESIDENT at the same time.  A sleep kernel in the collective's place does not exercise that; this one does: n_wg
// workgroups meet at a grid barrier (every one must have a CU), move the buffer through their registers chunk by chunk (sum over one
// rank = the values they found), meet again, and do not return before min_us have passed.  The barrier counter only grows (two
// arrivals per workgroup and launch): launches on one stream are ordered, which is how the callback transport uses it.  The spins
// are bounded (about a second): a stand-in that cannot become resident reports it through `stuck` instead of hanging the device.
__device__ unsigned long long g_standin_bar;
__global__ void k_standin_allreduce(unsigned long long* __restrict__ buf8, int64_t n8, unsigned long long base, double min_us,
                                    int32_t* __restrict__ stuck) {
  const unsigned long long t0 = wall_clock64();  // 100 MHz constant clock
  const unsigned long long n_wg = gridDim.x;
  __shared__ int ok;
  auto meet = [&](unsigned long long target) {
    if (threadIdx.x == 0) {
      __hip_atomic_fetch_add(&g_standin_bar, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      long spins = 0;
      ok = 1;
      while (__hip_atomic_load(&g_standin_bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
        __builtin_amdgcn_s_sleep(8);
        if (++spins > (1L << 22)) {
          ok = 0;
          if (stuck) atomicAdd(stuck, 1);
          break;
        }
      }
    }
    __syncthreads();
    return ok != 0;
  };
  const bool all_here = meet(base + n_wg);
  if (all_here)
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n8; i += (int64_t)n_wg * blockDim.x) {
      const unsigned long long v = __hip_atomic_load(buf8 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(buf8 + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  (void)meet(base + 2 * n_wg);
  if (threadIdx.x == 0)
    while ((double)(wall_clock64() - t0) * 0.01 < min_us) __builtin_amdgcn_s_sleep(16);
}
static unsigned long long g_standin_launches = 0;
