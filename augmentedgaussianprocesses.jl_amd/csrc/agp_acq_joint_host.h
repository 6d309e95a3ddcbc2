// agp_acq_joint_host.h -- host driver of the joint Monte-Carlo batch acquisition (kernels: agp_acq_joint.h; include/agp_hip.h
// "ACQUISITION FUNCTIONS", paragraph "Joint batches"): the argument checks that the two entry points share, which touch nothing, the
// workspaces of a call, and AcqJointDriver, which drives all the launches of agp_svgp_acquisition_joint and
// agp_svgp_acq_maximize_joint on the model's view (AcqModel) and with the passes and the ascent of AcqDriver (agp_acq_host.h).
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

// The joint entry points of one handle, next to its AcqDriver, whose particle state, group sums and ascent they use.  A set is q
// optimised points and the n pending ones.  Per chunk of floor(4096 / q) sets and pass: K*m and W of the chunk's points
// (acq_kstar_w), k_acqj_cov, k_acqj_set, and with the gradient k_acqj_weights, k_acq_contract on the weight rows and one finishing
// kernel: seven launches, nothing waits for the stream.  K*m, W and the record of the pending points are formed once per call, in
// workspaces of the call's own.  The order of the refusals is AcqDriver's.
struct AcqJointDriver {
  AcqJointWs acqj;

  agp_status begin(const AcqModel& M, const double* xp, int64_t ldp, int64_t n) {
    const AcqPred& pr = M.pred;
    if (n == 0) return AGP_OK;
    AGPCHK(acq_kstar_w(M, pr, xp, ldp, n, acqj.Kp, acqj.Wp));
    hipLaunchKernelGGL(agp::k_acqj_cov, dim3(1), dim3(agp::AJ_THREADS), 0, M.ctx->stream, 0, (int)n, (const double*)nullptr, (int64_t)0, xp,
                       ldp, (const double*)nullptr, (const double*)nullptr, (const double*)acqj.Kp, (const double*)acqj.Wp, pr.ld, pr.m,
                       pr.a, (int)M.D, M.scales, M.kind, M.variance, M.kdiag, (const double*)nullptr, acqj.pend);
    LAUNCHCHK(M.ctx);
    return AGP_OK;
  }
  // alpha (and, with grad, the groups' sums in M.part and the point-to-point term in acqj.cross) of ns sets whose np = ns q points are
  // the rows of x
  agp_status pass(const AcqModel& M, AcqDriver& dr, const agp::AcqParams& p, const double* x, int64_t ldx, const double* xp, int64_t ldp,
                  int64_t n, int64_t q, int64_t ns, const double* eps, int64_t lde, int64_t S, bool grad, double* alpha, int* ng) {
    const AcqPred& pr = M.pred;
    hipStream_t st = M.ctx->stream;
    const int64_t np = ns * q;
    AGPCHK(acq_kstar_w(M, pr, x, ldx, np, pr.Kstar, pr.W));
    hipLaunchKernelGGL(agp::k_acqj_cov, dim3((unsigned)ns), dim3(agp::AJ_THREADS), 0, st, (int)q, (int)n, x, ldx, xp, ldp,
                       (const double*)pr.Kstar, (const double*)pr.W, (const double*)acqj.Kp, (const double*)acqj.Wp, pr.ld, pr.m, pr.a,
                       (int)M.D, M.scales, M.kind, M.variance, M.kdiag, n > 0 ? (const double*)acqj.pend : (const double*)nullptr,
                       acqj.rec);
    hipLaunchKernelGGL(agp::k_acqj_set, dim3((unsigned)ns), dim3(agp::AJ_THREADS), 0, st, p, (int)(q + n), (int)S, eps, lde,
                       (const double*)acqj.rec, grad ? 1 : 0, alpha, acqj.bar, acqj.bad);
    LAUNCHCHK(M.ctx);
    if (grad) {
      hipLaunchKernelGGL(agp::k_acqj_weights, dim3((unsigned)((pr.m + agp::AJ_THREADS - 1) / agp::AJ_THREADS), (unsigned)ns),
                         dim3(agp::AJ_THREADS), 0, st, (int)q, (int)n, x, ldx, xp, ldp, (const double*)pr.W, (const double*)acqj.Wp, pr.ld,
                         pr.m, pr.a, (int)M.D, M.scales, M.kind, M.variance, (const double*)acqj.bar, acqj.V, pr.ld, acqj.cross);
      *ng = acq_contract_launch<true>(st, x, ldx, np, pr.Z, pr.m, M.D, M.scales, M.kind, M.variance, pr.a, (const double*)acqj.V, pr.ld,
                                      M.part, dr.acq.sc);
      LAUNCHCHK(M.ctx);
    }
    return AGP_OK;
  }

  static agp_status evaluate(SvgpBase& h, int l, const agp_acq_desc* d, const double* xp, int64_t ldp, int64_t n, int64_t q,
                             const double* xq, int64_t ldx, int64_t nsets, const double* eps, int64_t lde, int64_t S, double* alpha_out,
                             double* grad_out, int64_t ldg) {
    const char* who = "agp_svgp_acquisition_joint: ";
    const int64_t D = h.desc.D;
    agp::AcqParams p;
    AGPCHK(h.acq_check(who, l, d, &p));
    AGPCHK(acqj_check_args(h.ctx, who, p, D, xp, ldp, n, q, eps, lde, S));
    AGPCHK(acq_check_eval_out(h.ctx->err, who, "n_sets", "xq", D, nsets, xq, ldx, alpha_out, grad_out, ldg));
    if (nsets == 0) return AGP_OK;
    AcqModel M;
    AcqDriver* dr;
    AcqJointDriver* j;
    AGPCHK(h.acq_open(l, false, &M, &dr, &j));
    AGPCHK(j->acqj.ensure(M.ctx, M.mp, D));
    AGPCHK(j->begin(M, xp, ldp, n));
    const int64_t spc = agp::PG_CH / q;  // sets per chunk: a tuple never straddles two chunks
    for (int64_t s = 0; s < nsets; s += spc) {
      const int64_t ns = (nsets - s) < spc ? (nsets - s) : spc;
      int ng = 0;
      AGPCHK(j->pass(M, *dr, p, xq + s * q * ldx, ldx, xp, ldp, n, q, ns, eps, lde, S, grad_out != nullptr, alpha_out + s, &ng));
      if (grad_out) {
        hipLaunchKernelGGL(agp::k_acqj_grad, grid1(ns * q * D), dim3(256), 0, M.ctx->stream, ns * q, (int)D, ng, (const double*)M.part,
                           (const double*)j->acqj.cross, M.scales, grad_out + s * q * ldg, ldg);
        LAUNCHCHK(M.ctx);
      }
    }
    return AGP_OK;
  }
  static agp_status maximize(SvgpBase& h, int l, const agp_acq_desc* d, const double* xp, int64_t ldp, int64_t n, int64_t q,
                             const double* x0, int64_t ldx0, int64_t R, const double* eps, int64_t lde, int64_t S,
                             const agp_pw_ascent_opts* o, double* x_out, int64_t ldxo, double* a_out, double* best_x, int64_t ldb,
                             double* best_a, int64_t* best_idx) {
#pragma clang fp contract(off)
    const char* who = "agp_svgp_acq_maximize_joint: ";
    const int64_t D = h.desc.D;
    agp::AcqParams p;
    agp::PwAscentBox box;
    AGPCHK(h.acq_check(who, l, d, &p));
    AGPCHK(acqj_check_args(h.ctx, who, p, D, xp, ldp, n, q, eps, lde, S));
    AGPCHK(acq_check_ascent(h.ctx, who, D, x0, ldx0, R, AGP_ACQ_JOINT_MAX_Q, o, &box, "x_out", "ldxo", false, x_out, ldxo,
                            a_out || best_x || best_a || best_idx, best_x, ldb));
    AcqModel M;
    AcqDriver* dr;
    AcqJointDriver* j;
    AGPCHK(h.acq_open(l, true, &M, &dr, &j));
    AcqJointWs& w = j->acqj;
    AGPCHK(dr->acq.ensure_particles(M.ctx, R * q, D));
    AGPCHK(w.ensure(M.ctx, M.mp, D));
    AGPCHK(j->begin(M, xp, ldp, n));
    AGPCHK(dr->ascend(
        M, box, o, x0, ldx0, R, q,
        [&](double* x, int64_t s, int64_t ns, bool fin, int* ng) {
          return j->pass(M, *dr, p, x, D, xp, ldp, n, q, ns, eps, lde, S, !fin, dr->acq.A + s, ng);
        },
        [&](double* x, int64_t, int64_t ns, int ng, bool fin, double c1, double c2) -> agp_status {
          if (fin) return AGP_OK;  // (the last pass has left alpha at the final tuple)
          hipLaunchKernelGGL(agp::k_acqj_step, grid1(ns * q * D), dim3(256), 0, M.ctx->stream, ns * q, (int)D, ng, (const double*)M.part,
                             (const double*)w.cross, M.scales, o->beta1, o->beta2, c1, c2, o->eps, box, x, dr->acq.mo, dr->acq.vo);
          LAUNCHCHK(M.ctx);
          return AGP_OK;
        }));
    if (best_x || best_a || best_idx) {  // a tuple is one row of q D values for the best-start rule
      hipLaunchKernelGGL(agp::k_pw_ascent_best, dim3(1), dim3(256), 0, M.ctx->stream, (const double*)dr->acq.X, (const double*)dr->acq.A, R,
                         q * D, 1.0, best_x ? w.bx : (double*)nullptr, q * D, best_a, best_idx);
      LAUNCHCHK(M.ctx);
      if (best_x)
        HIPCHK(M.ctx, hipMemcpy2DAsync(best_x, sizeof(double) * ldb, w.bx, sizeof(double) * D, sizeof(double) * D, q,
                                       hipMemcpyDeviceToDevice, M.ctx->stream));
    }
    return dr->copy_out(M, R * q, R, x_out, ldxo, a_out);
  }
};
