// agp_acq_joint_host.h -- host driver of the joint Monte-Carlo batch acquisition (kernels: agp_acq_joint.h; include/agp_hip.h
// "ACQUISITION FUNCTIONS", paragraph "Joint batches"): the argument checks that the two entry points share, which touch nothing, and
// the workspaces of a call.  Svgp<T>::acquisition_joint / acq_maximize_joint (agp_capi.hip) drive the launches with the predictor's
// workspaces, as agp_acq_host.h's callers do.
#pragma once
#include <string>

#include "agp_acq_host.h"
#include "agp_acq_joint.h"
#include "agp_ctx.h"

// kind, q, n, S, eps, lde and the pending points: AGP_ERR_UNSUPPORTED for the kinds that have no joint form, AGP_ERR_INVALID otherwise
static agp_status acqj_check_args(agp_ctx* ctx, const char* who, const agp::AcqParams& p, int64_t D, const void* xp, int64_t ldp,
                                  int64_t n, int64_t q, const void* eps, int64_t lde, int64_t S) {
  auto invalid = [&](const char* what) {
    ctx->err = std::string(who) + what;
    return AGP_ERR_INVALID;
  };
  if (p.kind != AGP_ACQ_UCB && p.kind != AGP_ACQ_EI) {
    ctx->err = std::string(who) + (p.kind == AGP_ACQ_PI       ? "AGP_ACQ_PI"
                                   : p.kind == AGP_ACQ_LOG_EI ? "AGP_ACQ_LOG_EI"
                                                              : "AGP_ACQ_LOG_PI") +
               " has no joint form here (the joint PI has a zero gradient almost everywhere, the log kinds need a smoothed maximum): "
               "AGP_ACQ_EI or AGP_ACQ_UCB";
    return AGP_ERR_UNSUPPORTED;
  }
  if (q < 1) return invalid("q >= 1");
  if (n < 0) return invalid("n_pending >= 0");
  if (q > AGP_ACQ_JOINT_MAX_Q || n > AGP_ACQ_JOINT_MAX_Q || q + n > AGP_ACQ_JOINT_MAX_Q)
    return invalid("q + n_pending <= AGP_ACQ_JOINT_MAX_Q (16)");
  if (S < 1 || S > agp::AJ_SMAX) return invalid("S must lie in [1, 4096]");
  if (!eps) return invalid("eps must be given");
  if (lde < q + n) return invalid("lde >= q + n_pending");
  if (n > 0 && !xp) return invalid("xp must be given when n_pending > 0");
  if (n > 0 && ldp < D) return invalid("ldp >= D");
  return AGP_OK;
}

// What a joint call keeps on the handle, allocated once (every size is bounded by the chunk of 4096 particles, the interface limit
// of 16 members and m): K*m and W of the pending points with their own record, the sets' records (C, mu) and (C-bar, mu-bar), the
// weight rows, the point-to-point term, the best tuple, and the pivot latch that agp_svgp_check_status reads.
struct AcqJointWs {
  double *Kp = nullptr, *Wp = nullptr, *pend = nullptr;  // [64][ld] x 2, [AJ_REC]
  double *rec = nullptr, *bar = nullptr;                 // [4096][AJ_REC] each
  double *V = nullptr, *cross = nullptr, *bx = nullptr;  // [4096][ld], [4096][D], [16 D]
  int32_t* bad = nullptr;
  agp_status ensure(agp_ctx* ctx, int64_t ld, int64_t D) {
    if (V) return AGP_OK;
    auto need = [&](double** p, int64_t n) { return *p ? AGP_OK : dmalloc(ctx, p, n); };  // (a call after a failed one goes on)
    AGPCHK(need(&Kp, 64 * ld));
    AGPCHK(need(&Wp, 64 * ld));
    AGPCHK(need(&pend, agp::AJ_REC));
    AGPCHK(need(&rec, (int64_t)agp::PG_CH * agp::AJ_REC));
    AGPCHK(need(&bar, (int64_t)agp::PG_CH * agp::AJ_REC));
    AGPCHK(need(&cross, (int64_t)agp::PG_CH * D));
    AGPCHK(need(&bx, (int64_t)agp::AJ_Q * D));
    if (!bad) {
      AGPCHK(dmalloc(ctx, &bad, 1));
      HIPCHK(ctx, hipMemsetAsync(bad, 0, sizeof(int32_t), ctx->stream));
    }
    AGPCHK(need(&V, (int64_t)agp::PG_CH * ld));  // (last: V != NULL says that all of them stand)
    return AGP_OK;
  }
  ~AcqJointWs() {
    for (double* p : {Kp, Wp, pend, rec, bar, V, cross, bx})
      if (p) (void)hipFree(p);
    if (bad) (void)hipFree(bad);
  }
};
