// agp_acq_check.h -- the checks of the acquisition entry points on their outputs and leading dimensions (include/agp_hip.h
// "ACQUISITION FUNCTIONS"), one for the evaluations and one for the maximisers, with the words that differ between the entry points
// as arguments.  They touch nothing and call nothing of HIP, so the header also compiles for the host alone (any C++ compiler):
// tests/c_host/acq_check_messages.cpp prints every message and tests/test_acq_host.py compares them with the interface's.
#pragma once
#include <stdint.h>

#include <string>

#include "../../include/agp_hip.h"

// the points and outputs of an evaluation; `count` and `rows` name its first two arguments ("n_t", "xt" or "n_sets", "xq")
static agp_status acq_check_eval_out(std::string& err, const char* who, const char* count, const char* rows, int64_t D, int64_t n,
                                     const void* x, int64_t ldx, const void* alpha_out, const void* grad_out, int64_t ldg) {
  if (n < 0 || ldx < D || (grad_out && ldg < D) || (n > 0 && (!x || !alpha_out))) {
    err = std::string(who) + count + " >= 0, " + rows + " and alpha_out must not be NULL, ldx >= D, ldg >= D when grad_out is given";
    return AGP_ERR_INVALID;
  }
  return AGP_OK;
}

// the starts and outputs of a maximiser, after x0 and the options.  x_out with its leading dimension ldxo goes by the names xname and
// ldname; it is either the one output that must be there (x_required) or one of several, of which other_out says whether any is
// given.  A start holds up to `per` particles (1, or AGP_ACQ_JOINT_MAX_Q), all of which a 32-bit count must hold.  best_x, where the
// caller pitches it, has the leading dimension ldb.
static agp_status acq_check_max_out(std::string& err, const char* who, int64_t D, int64_t R, int64_t per, int64_t ldx0,
                                    const char* xname, const char* ldname, bool x_required, const void* x_out, int64_t ldxo,
                                    bool other_out, const void* best_x, int64_t ldb) {
  auto invalid = [&](const std::string& what) {
    err = std::string(who) + what;
    return AGP_ERR_INVALID;
  };
  if (x_required && !x_out) return invalid(std::string(xname) + " must be given");
  if (!x_out && !other_out) return invalid("at least one output must be given");
  if (R < 1 || R >= ((int64_t)1 << 31) / per)
    return invalid("n_starts >= 1 and " + (per > 1 ? "n_starts * " + std::to_string(per) + " " : std::string()) + "below 2^31");
  if (ldx0 < D) return invalid("ldx0 >= D");
  if (x_out && ldxo < D) return invalid(std::string(ldname) + " >= D" + (x_required ? "" : std::string(" when ") + xname + " is given"));
  if (best_x && ldb < D) return invalid("ldb >= D when best_x is given");
  return AGP_OK;
}
