// agp_acq_host.h -- host driver of the acquisition functions (kernels: agp_acq.h; include/agp_hip.h "ACQUISITION FUNCTIONS"): the
// argument checks of agp_acq_desc and agp_pw_ascent_opts, which touch nothing, agp_acq_moments, the launch of k_acq_contract and the
// particle state of the ascent.  Svgp<T>::acquisition / acq_maximize (agp_capi.hip) drive them with the predictor's workspaces.
#pragma once
#include <cmath>
#include <string>

#include "agp_acq.h"
#include "agp_ctx.h"

// desc -> AcqParams, or AGP_ERR_INVALID with a message
static agp_status acq_check_desc(agp_ctx* ctx, const char* who, const agp_acq_desc* d, agp::AcqParams* out) {
  auto invalid = [&](const std::string& what) {
    ctx->err = std::string(who) + what;
    return AGP_ERR_INVALID;
  };
  if (!d) return invalid("desc must be given");
  if (d->kind != AGP_ACQ_UCB && d->kind != AGP_ACQ_EI && d->kind != AGP_ACQ_PI)
    return invalid("unknown kind (AGP_ACQ_UCB, AGP_ACQ_EI or AGP_ACQ_PI)");
  if (!std::isfinite(d->beta) || !std::isfinite(d->best) || !std::isfinite(d->xi)) return invalid("beta, best and xi must be finite");
  if (d->beta < 0.0) return invalid("beta >= 0");
  if (d->xi < 0.0) return invalid("xi >= 0");
  out->kind = d->kind;
  out->s = d->minimize ? -1.0 : 1.0;
  out->beta = d->beta, out->best = d->best, out->xi = d->xi;
  return AGP_OK;
}

// the checks of agp_pathwise_maximize on the options it shares (pw_maximize), in its words; the direction and the shared starts
// belong to the paths and must be 0 here
static agp_status acq_check_opts(agp_ctx* ctx, const char* who, int64_t D, const agp_pw_ascent_opts* o, agp::PwAscentBox* box) {
  auto invalid = [&](const std::string& what) {
    ctx->err = std::string(who) + what;
    return AGP_ERR_INVALID;
  };
  if (!o) return invalid("opts must be given");
  if (o->minimize != 0 || o->x0_shared != 0) return invalid("opts->minimize and opts->x0_shared must be 0 (the direction is agp_acq_desc.minimize)");
  if (o->steps < 0 || o->steps > 65536) return invalid("steps must lie in [0, 65536]");
  if (!(o->beta1 >= 0.0 && o->beta1 < 1.0) || !(o->beta2 >= 0.0 && o->beta2 < 1.0)) return invalid("0 <= beta1, beta2 < 1");
  if (!(o->eps > 0.0) || !std::isfinite(o->eps)) return invalid("eps must be finite and > 0");
  if (!o->lo_host || !o->hi_host || !o->lr_host) return invalid("lo_host, hi_host and lr_host must be given");
  *box = agp::PwAscentBox{};
  for (int64_t d = 0; d < D; ++d) {
    const double lo = o->lo_host[d], hi = o->hi_host[d], lr = o->lr_host[d];
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo <= hi))
      return invalid("the bounds must be finite with lo <= hi (dimension " + std::to_string(d) + ")");
    if (!std::isfinite(lr) || !(lr > 0.0)) return invalid("the step sizes must be finite and > 0 (dimension " + std::to_string(d) + ")");
    box->lo[d] = lo, box->hi[d] = hi, box->lr[d] = lr;
  }
  return AGP_OK;
}

static agp_status acq_moments(agp_ctx* ctx, const agp_acq_desc* d, int64_t n, const double* mu, const double* var, double* alpha,
                              double* dmu, double* dvar) {
  const char* who = "agp_acq_moments: ";
  agp::AcqParams p;
  AGPCHK(acq_check_desc(ctx, who, d, &p));
  if (n < 0 || (n > 0 && (!mu || !var || !alpha))) {
    ctx->err = std::string(who) + "n >= 0; mu, var and alpha_out must not be NULL";
    return AGP_ERR_INVALID;
  }
  if (n == 0) return AGP_OK;
  hipLaunchKernelGGL(agp::k_acq_moments, grid1(n), dim3(256), 0, ctx->stream, p, n, mu, var, alpha, dmu, dvar);
  LAUNCHCHK(ctx);
  return AGP_OK;
}

// k_acq_contract of nc <= 4096 particles; returns the number of column groups (what k_acq_step / k_acq_finish add up)
template <bool GRAD>
static int acq_contract_launch(hipStream_t s, const double* xs, int64_t ldx, int64_t nc, const double* Z, int64_t m, int64_t D,
                               const double* scales, int kind, double variance, const double* a, const double* W, int64_t ldw,
                               double* part, double* sc) {
  const int dpt = D <= 4 ? 1 : (D <= 16 ? 4 : (D <= 32 ? 8 : 16));
  const int64_t tpg = agp::pg_tiles_per_group(m, dpt), ntile = (m + agp::pg_ct(dpt) - 1) / agp::pg_ct(dpt), ng = (ntile + tpg - 1) / tpg;
  const dim3 grid((unsigned)((nc + agp::PG_RT - 1) / agp::PG_RT), (unsigned)ng), blk(agp::PG_THREADS);
#define AGP_ACQ_LAUNCH(DPT) \
  hipLaunchKernelGGL((agp::k_acq_contract<DPT, GRAD>), grid, blk, 0, s, xs, ldx, nc, Z, D, m, (int)D, scales, kind, variance, a, W, ldw, tpg, part, sc)
  if (dpt == 1) AGP_ACQ_LAUNCH(1);
  else if (dpt == 4) AGP_ACQ_LAUNCH(4);
  else if (dpt == 8) AGP_ACQ_LAUNCH(8);
  else AGP_ACQ_LAUNCH(16);
#undef AGP_ACQ_LAUNCH
  return (int)ng;
}

// What the ascent keeps on the handle: the groups' scalar sums of one chunk, the ADAM moments of one chunk, and the iterate and alpha
// of every particle of the call (grown by the call that has more starts than any before: the one place that may wait for the device)
struct AcqState {
  double *sc = nullptr, *mo = nullptr, *vo = nullptr;  // [2][PG_MAXGROUPS][4096] ; [4096][D] each
  double *X = nullptr, *A = nullptr;                  // [cap][D], [cap]
  int64_t cap = 0;
  agp_status ensure_chunk(agp_ctx* ctx, int64_t D, bool ascent) {
    if (!sc) AGPCHK(dmalloc(ctx, &sc, 2 * (int64_t)agp::PG_MAXGROUPS * agp::PG_CH));
    if (ascent && !mo) AGPCHK(dmalloc(ctx, &mo, (int64_t)agp::PG_CH * D));
    if (ascent && !vo) AGPCHK(dmalloc(ctx, &vo, (int64_t)agp::PG_CH * D));
    return AGP_OK;
  }
  agp_status ensure_particles(agp_ctx* ctx, int64_t R, int64_t D) {
    if (R <= cap) return AGP_OK;
    for (double** q : {&X, &A})
      if (*q) (void)hipFree(*q), *q = nullptr;
    cap = 0;
    AGPCHK(dmalloc(ctx, &X, R * D));
    AGPCHK(dmalloc(ctx, &A, R));
    cap = R;
    return AGP_OK;
  }
  ~AcqState() {
    for (double* q : {sc, mo, vo, X, A})
      if (q) (void)hipFree(q);
  }
};
