// The point function of the acquisition kinds that are evaluated in logarithms (AGP_ACQ_LOG_EI, AGP_ACQ_LOG_PI; include/agp_hip.h
// "ACQUISITION FUNCTIONS").  Float64 only.  With sigma = sqrt(var), imp = s (mu - best) - xi, z = imp / sigma,
// phi(z) = exp(-z^2 / 2) / sqrt(2 pi), Phi(z) = erfc(-z / sqrt 2) / 2, h(z) = phi(z) + z Phi(z) and the Mills ratio R(z) = Phi(z) / phi(z):
//   kind     alpha                    d alpha / d mu          d alpha / d sigma           (d alpha / d var = that / (2 sigma))
//   LogEI    log sigma + log h(z)     s Phi / (sigma h)       phi / (sigma h)
//   LogPI    log Phi(z)               s phi / (sigma Phi)     -z phi / (sigma Phi)
// EI and PI underflow to 0, with a zero gradient, for z below about -38; their logarithms are finite with a useful gradient as far as
// z^2 / 2 is a double.  Two branches:
//   z > -3    the direct expressions; Phi from erfc, never from 1 + erf; log Phi for z > 0 is log1p(-Phi(-z)).  h = phi + z Phi has
//             lost about one digit to cancellation at z = -3.
//   z <= -3   t = -z and Laplace's continued fraction for the Mills ratio, cut after the partial numerator n and evaluated from its
//             tail with one division per term; n = 60 for t < 5, 32 for t < 12, 12 beyond (acq_log_cf_terms: the cut changes c by less
//             than 2.5e-17 of itself in each range):
//               c = 1 / (t + 2 / (t + 3 / (t + ... )))      R = 1 / (t + c)      h / phi = 1 - t R = c R   (no cancellation)
//               log h = -z^2 / 2 - log sqrt(2 pi) + log c + log R          log Phi = -z^2 / 2 - log sqrt(2 pi) + log R
//               Phi / h = 1 / c        phi / h = 1 / (c R) = (t + c) / c        phi / Phi = 1 / R = t + c
//             -z^2 / 2 is formed as (-z / 2) z: it overflows only where the exact value lies below -DBL_MAX.
// The trip count is one of three by the range of t, there is no scratch, and only erfc, exp, log, log1p and sqrt are called: the
// header also compiles for the host alone (any C++ compiler), which is how the host suite checks this very code against an
// extended-precision reference.
// var <= 0 takes the limit: LogEI alpha = log imp, d alpha / d mu = s / imp where imp > 0, else alpha = -inf and d alpha / d mu = 0;
// LogPI alpha = 0 where imp > 0, else -inf, d alpha / d mu = 0; the var term is 0 in both.  A NaN moment gives NaN in all three.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AGP_ACQ_LOG_HD __host__ __device__
#else
#define AGP_ACQ_LOG_HD
#endif

namespace agp {

constexpr int ACQ_LOG_EI = 5, ACQ_LOG_PI = 6;  // AGP_ACQ_LOG | AGP_ACQ_EI, AGP_ACQ_LOG | AGP_ACQ_PI
constexpr double ACQ_LOG_BRANCH = -3.0;        // z <= this: the continued fraction

// the last partial numerator of the continued fraction at t >= 3: the fewest of {60, 32, 12} that leave the cut below eps / 8
AGP_ACQ_LOG_HD inline int acq_log_cf_terms(double t) { return t < 5.0 ? 60 : (t < 12.0 ? 32 : 12); }

// kind: ACQ_LOG_EI or ACQ_LOG_PI; s: +1, or -1 with minimize
AGP_ACQ_LOG_HD inline void acq_log_point(int kind, double s, double best, double xi, double mu, double var, double& alpha, double& dmu,
                                         double& dvar) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (mu != mu || var != var) {
    alpha = dmu = dvar = __builtin_nan("");
    return;
  }
  const double imp = s * (mu - best) - xi;
  if (!(var > 0.0)) {
    dvar = 0.0;
    if (kind == ACQ_LOG_EI) alpha = imp > 0.0 ? log(imp) : -__builtin_inf(), dmu = imp > 0.0 ? s / imp : 0.0;
    else alpha = imp > 0.0 ? 0.0 : -__builtin_inf(), dmu = 0.0;
    return;
  }
  const double sg = sqrt(var);
  const double z = imp / sg;
  double dsg;
  if (z > ACQ_LOG_BRANCH) {
    const double phi = 0.39894228040143267794 * exp(-0.5 * (z * z));
    if (kind == ACQ_LOG_EI) {
      const double Phi = 0.5 * erfc(-z * 0.70710678118654752440);
      const double h = phi + z * Phi;
      alpha = log(sg) + log(h);
      dmu = s * Phi / (sg * h);
      dsg = phi / (sg * h);
    } else {
      const bool up = z > 0.0;
      const double Q = 0.5 * erfc((up ? z : -z) * 0.70710678118654752440);  // the smaller of Phi(z) and Phi(-z)
      const double Phi = up ? 1.0 - Q : Q;
      alpha = up ? log1p(-Q) : log(Q);
      dmu = s * phi / (sg * Phi);
      dsg = -z * phi / (sg * Phi);
    }
  } else {
    const double t = -z;
    double u = 0.0;
    for (int k = acq_log_cf_terms(t); k >= 2; --k) u = (double)k / (t + u);
    const double c = 1.0 / (t + u);
    const double tc = t + c;  // 1 / R
    const double tail = (-0.5 * z) * z - 0.91893853320467274178;  // log phi(z)
    if (kind == ACQ_LOG_EI) {
      alpha = tail + (log(c) - log(tc) + log(sg));
      dmu = s / (sg * c);
      dsg = tc / (sg * c);
    } else {
      alpha = tail - log(tc);
      dmu = s * tc / sg;
      dsg = t * tc / sg;
    }
  }
  dvar = dsg / (2.0 * sg);
}

}  // namespace agp
