// agp_lpd_host.h -- host driver of the log predictive density (kernels: agp_lpd.h): which likelihoods it takes (lpd_lik_ok), the
// likelihood's parameters as the kernel takes them (lpd_params), the Gauss-Hermite rule kept on the device (LpdRule), one launch of
// k_predict_lpd over a chunk of points (lpd_launch) and the kernel's failure words as status and message (lpd_failure).  Used by
// SvgpBase::lpd_stream (agp_svgp_base.h) and agp_log_predictive (agp_capi.hip).
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "agp_ctx.h"
#include "agp_lpd.h"

// ---- log predictive density (include/agp_hip.h, "LOG PREDICTIVE DENSITY"; device code in agp_lpd.h) ----------------------------------
static bool lpd_lik_ok(int kind) {
  return kind == AGP_LIK_GAUSSIAN || kind == AGP_LIK_LAPLACE || lpd_is_quad(kind) || lpd_is_multiclass(kind);
}
// the likelihood's parameters as the kernel takes them, constants formed here (lgamma)
static agp_status lpd_params(agp_ctx* ctx, const char* who, const agp_lik_desc& lik, LpdParams* P) {
  P->p0 = lik.p0, P->p1 = lik.p1, P->c0 = 0.0;
  const int k = lik.kind;
  const bool need_p0 = k == AGP_LIK_GAUSSIAN || k == AGP_LIK_LAPLACE || k == AGP_LIK_POISSON || k == AGP_LIK_NEGBINOMIAL;
  if ((need_p0 && !(lik.p0 > 0)) || (k == AGP_LIK_STUDENTT && !(lik.p0 > 0.5 && lik.p1 > 0))) {
    ctx->err = std::string(who) + ": Gaussian sigma2, Laplace beta, Poisson lambda and NegBinomial r must be positive, StudentT needs "
               "nu > 0.5 and sigma > 0";
    return AGP_ERR_INVALID;
  }
  if (k == AGP_LIK_STUDENTT)  // studentt.jl:43-46 as written (nvi_lconst)
    P->c0 = std::lgamma(0.5 * (lik.p0 + 1.0)) - 0.5 * std::log(lik.p0 * 3.141592653589793) - std::lgamma(0.5 * lik.p0);
  if (k == AGP_LIK_LAPLACE) P->c0 = -std::log(4.0 * lik.p0);
  if (k == AGP_LIK_NEGBINOMIAL) P->c0 = -std::lgamma(lik.p0);
  return AGP_OK;
}
// The Gauss-Hermite rule on the device, nodes | log weights, uploaded only when the caller's rule changes.
struct LpdRule {
  double* dev = nullptr;
  int cap = 0;
  std::vector<double> nodes, weights, up;
  ~LpdRule() {
    if (dev) (void)hipFree(dev);
  }
  agp_status ensure(agp_ctx* ctx, const char* who, hipStream_t s, const double* x, const double* w, int nn) {
    if (!x || !w || nn < 1 || nn > 4096) {
      ctx->err = std::string(who) + ": this likelihood needs the Gauss-Hermite nodes and weights, 1 <= n_nodes <= 4096";
      return AGP_ERR_INVALID;
    }
    if (dev && (int)nodes.size() == nn && !std::memcmp(nodes.data(), x, sizeof(double) * nn) &&
        !std::memcmp(weights.data(), w, sizeof(double) * nn))
      return AGP_OK;
    for (int j = 0; j < nn; ++j)
      if (!std::isfinite(x[j]) || !(w[j] >= 0.0) || !std::isfinite(w[j])) {
        ctx->err = std::string(who) + ": the nodes must be finite and the weights finite and non-negative";
        return AGP_ERR_INVALID;
      }
    nodes.clear();  // (nothing counts as cached until the upload has been enqueued)
    // an earlier upload may still read the staging vector: the stream is drained before it is rewritten (a change of rule is rare)
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (nn > cap) {
      if (dev) (void)hipFree(dev);
      dev = nullptr, cap = 0;
      AGPCHK(dmalloc(ctx, &dev, 2 * (int64_t)nn));
      cap = nn;
    }
    up.assign(x, x + nn);
    for (int j = 0; j < nn; ++j) up.push_back(std::log(w[j]));  // (a zero weight: -inf, the node is skipped)
    HIPCHK(ctx, hipMemcpyAsync(dev, up.data(), sizeof(double) * 2 * nn, hipMemcpyHostToDevice, s));
    nodes.assign(x, x + nn);
    weights.assign(w, w + nn);
    return AGP_OK;
  }
};
// one launch of k_predict_lpd over nc points that start at stream position `base`; part points at the launch's first workgroup
template <typename T>
static agp_status lpd_launch(agp_ctx* ctx, hipStream_t s, int kind, int64_t nc, int64_t base, int nl, int64_t ld, const LpdParams& P,
                             const T* lstate, const void* y, const T* mu, const T* var, const double* quad, int nn, T* lpd_out,
                             double* part, unsigned long long* bad) {
  const unsigned gw = (unsigned)((nc + lpd_points_per_block(kind) - 1) / lpd_points_per_block(kind));
#define AGP_LPD_CASE(K)                                                                                                            \
  case K:                                                                                                                          \
    hipLaunchKernelGGL((k_predict_lpd<T, K>), dim3(gw), dim3(LPD_THREADS), 0, s, nc, base, nl, ld, P, lstate, (const T*)y,          \
                       (const int32_t*)y, mu, var, quad, nn, lpd_out, part, bad);                                                 \
    break;
  switch (kind) {
    AGP_LPD_CASE(LIK_GAUSSIAN)
    AGP_LPD_CASE(LIK_LOGISTIC)
    AGP_LPD_CASE(LIK_STUDENTT)
    AGP_LPD_CASE(LIK_LSM)
    AGP_LPD_CASE(LIK_LAPLACE)
    AGP_LPD_CASE(LIK_BSVM)
    AGP_LPD_CASE(LIK_POISSON)
    AGP_LPD_CASE(LIK_NEGBIN)
    AGP_LPD_CASE(LIK_SOFTMAX)
    default:
      ctx->err = "log predictive density: unknown likelihood kind";
      return AGP_ERR_UNSUPPORTED;
  }
#undef AGP_LPD_CASE
  LAUNCHCHK(ctx);
  return AGP_OK;
}
// the two failure words (as k_lpd_reduce leaves them) -> status and message
static agp_status lpd_failure(agp_ctx* ctx, const char* who, const double* h) {
  if (h[1] >= 0.0) {
    ctx->err = std::string(who) + ": var_f is not positive (or a moment is not finite) at point " + std::to_string((int64_t)h[1]) +
               " of the stream (K~ has negative values)";
    return AGP_ERR_NEG_KTILDE;
  }
  if (h[2] >= 0.0) {
    ctx->err = std::string(who) + ": a target the likelihood cannot take (class index outside the likelihood's classes, a count that "
               "is not a non-negative integer, a binary label that is not +-1) at point " + std::to_string((int64_t)h[2]) +
               " of the stream";
    return AGP_ERR_LABELS;
  }
  return AGP_OK;
}
