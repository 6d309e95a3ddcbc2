// The point function of the log acquisition kinds (csrc/agp_acq_log.h) compiled for the host alone: reads lines
//   kind s best xi mu var        (kind 5 = LogEI, 6 = LogPI; the numbers in any form strtod reads, hex floats included)
// from standard input and prints alpha, d alpha / d mu, d alpha / d var of each as hex floats.  tests/test_acq_log_host.py builds
// and drives it.
#include <stdio.h>
#include <stdlib.h>

#include "agp_acq_log.h"

int main() {
  char line[512];
  while (fgets(line, sizeof line, stdin)) {
    char* p = line;
    const int kind = (int)strtol(p, &p, 10);
    double v[5];
    for (double& x : v) x = strtod(p, &p);
    double alpha, dmu, dvar;
    agp::acq_log_point(kind, v[0], v[1], v[2], v[3], v[4], alpha, dmu, dvar);
    printf("%a %a %a\n", alpha, dmu, dvar);
  }
  return 0;
}
