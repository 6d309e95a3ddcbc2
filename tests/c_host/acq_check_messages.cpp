// The checks of the acquisition entry points on their outputs (csrc/agp_acq_check.h) compiled for the host alone: calls them as the
// six entry points do, with D = 3 and one fault at a time (or several, to show which is named first), and prints one line per call:
//   label <tab> status <tab> message
// tests/test_acq_check_host.py builds it and compares the lines with the messages of include/agp_hip.h's entry points.
#include <stdio.h>

#include "agp_acq_check.h"

static const int64_t D = 3;
static double buf[8];

static void show(const char* label, agp_status s, const std::string& err) { printf("%s\t%d\t%s\n", label, (int)s, err.c_str()); }

// an evaluation: agp_svgp_acquisition and agp_svgp_acquisition_pending say (n_t, xt), agp_svgp_acquisition_joint (n_sets, xq)
static void eval(const char* label, const char* who, bool joint, int64_t n, const void* x, int64_t ldx, const void* alpha,
                 const void* grad, int64_t ldg) {
  std::string err;
  const agp_status s = acq_check_eval_out(err, who, joint ? "n_sets" : "n_t", joint ? "xq" : "xt", D, n, x, ldx, alpha, grad, ldg);
  show(label, s, err);
}

struct Max {
  int64_t R = 4, ldx0 = D, ldxo = D, ldb = D;
  const void *x_out = buf, *a_out = nullptr, *best_x = nullptr;
};
// the three maximisers, with the arguments that AcqDriver::maximize, maximize_batch and AcqJointDriver::maximize pass
static void plain(const char* label, const Max& m) {
  std::string err;
  show(label, acq_check_max_out(err, "agp_svgp_acq_maximize: ", D, m.R, 1, m.ldx0, "x_out", "ldxo", false, m.x_out, m.ldxo,
                                m.a_out || m.best_x, nullptr, 0), err);
}
static void batch(const char* label, const Max& m) {
  std::string err;
  show(label, acq_check_max_out(err, "agp_svgp_acq_maximize_batch: ", D, m.R, 1, m.ldx0, "xb_out", "ldxb", true, m.x_out, m.ldxo, false,
                                nullptr, 0), err);
}
static void joint(const char* label, const Max& m) {
  std::string err;
  show(label, acq_check_max_out(err, "agp_svgp_acq_maximize_joint: ", D, m.R, AGP_ACQ_JOINT_MAX_Q, m.ldx0, "x_out", "ldxo", false, m.x_out,
                                m.ldxo, m.a_out || m.best_x, m.best_x, m.ldb), err);
}

int main() {
  const int64_t two31 = (int64_t)1 << 31;
  eval("eval ok", "agp_svgp_acquisition: ", false, 5, buf, D, buf, buf, D);
  eval("eval empty", "agp_svgp_acquisition: ", false, 0, nullptr, D, nullptr, nullptr, 0);
  eval("eval no grad, ldg unused", "agp_svgp_acquisition: ", false, 5, buf, D, buf, nullptr, 0);
  eval("eval n < 0", "agp_svgp_acquisition: ", false, -1, buf, D, buf, nullptr, 0);
  eval("eval xt NULL", "agp_svgp_acquisition: ", false, 5, nullptr, D, buf, nullptr, 0);
  eval("eval alpha NULL", "agp_svgp_acquisition: ", false, 5, buf, D, nullptr, nullptr, 0);
  eval("eval ldx", "agp_svgp_acquisition: ", false, 5, buf, D - 1, buf, nullptr, 0);
  eval("eval ldx, empty", "agp_svgp_acquisition: ", false, 0, nullptr, D - 1, nullptr, nullptr, 0);
  eval("eval ldg", "agp_svgp_acquisition: ", false, 5, buf, D, buf, buf, D - 1);
  eval("pending ldg", "agp_svgp_acquisition_pending: ", false, 5, buf, D, buf, buf, D - 1);
  eval("pending ok", "agp_svgp_acquisition_pending: ", false, 5, buf, D + 2, buf, buf, D + 1);
  eval("joint n < 0", "agp_svgp_acquisition_joint: ", true, -1, buf, D, buf, nullptr, 0);
  eval("joint xq NULL", "agp_svgp_acquisition_joint: ", true, 1, nullptr, D, buf, nullptr, 0);
  eval("joint ok", "agp_svgp_acquisition_joint: ", true, 1, buf, D, buf, nullptr, 0);

  Max m;
  plain("max ok", m);
  m = Max(), m.x_out = nullptr, m.a_out = buf, m.ldxo = 0;
  plain("max a_out alone, ldxo unused", m);
  m = Max(), m.x_out = nullptr, m.R = 0, m.ldx0 = 0;
  plain("max no output (first of three)", m);
  m = Max(), m.R = 0, m.ldx0 = 0, m.ldxo = 0;
  plain("max n_starts 0 (first of three)", m);
  m = Max(), m.R = two31;
  plain("max n_starts 2^31", m);
  m = Max(), m.R = two31 - 1;
  plain("max n_starts 2^31 - 1", m);
  m = Max(), m.ldx0 = D - 1, m.ldxo = D - 1;
  plain("max ldx0 (first of two)", m);
  m = Max(), m.ldxo = D - 1;
  plain("max ldxo", m);

  m = Max();
  batch("batch ok", m);
  m = Max(), m.x_out = nullptr, m.R = 0;
  batch("batch no xb_out (first of two)", m);
  m = Max(), m.R = two31;
  batch("batch n_starts 2^31", m);
  m = Max(), m.ldx0 = D - 1, m.ldxo = D - 1;
  batch("batch ldx0 (first of two)", m);
  m = Max(), m.ldxo = D - 1;
  batch("batch ldxb", m);

  m = Max(), m.best_x = buf;
  joint("jmax ok", m);
  m = Max(), m.x_out = nullptr, m.R = 0;
  joint("jmax no output (first of two)", m);
  m = Max(), m.R = two31 / 16;
  joint("jmax n_starts 2^27", m);
  m = Max(), m.R = two31 / 16 - 1;
  joint("jmax n_starts 2^27 - 1", m);
  m = Max(), m.R = 0;
  joint("jmax n_starts 0", m);
  m = Max(), m.ldx0 = D - 1, m.ldxo = D - 1, m.best_x = buf, m.ldb = D - 1;
  joint("jmax ldx0 (first of three)", m);
  m = Max(), m.ldxo = D - 1, m.best_x = buf, m.ldb = D - 1;
  joint("jmax ldxo (first of two)", m);
  m = Max(), m.best_x = buf, m.ldb = D - 1;
  joint("jmax ldb", m);
  m = Max(), m.ldb = D - 1;
  joint("jmax no best_x, ldb unused", m);
  return 0;
}
