// Prints the library's host-side dense differentiation matrix (csrc/diffmat.cpp: diffmat_dense_host) for the line lengths
// given on the command line: one line "P" followed by P * P entries as hexadecimal floats (exact), row-major.
// Built and run by tests/test_linewise_host.py; needs no GPU.
#include "sweep.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace chebhip;

int main(int argc, char **argv) {
  for (int a = 1; a < argc; a++) {
    const int P = atoi(argv[a]);
    if (P < 2 || P > 4096) { printf("%d failed\n", P); continue; }
    std::vector<double> D((size_t)P * P);
    diffmat_dense_host(P, D.data());
    printf("%d\n", P);
    for (size_t k = 0; k < D.size(); k++) printf("%a\n", D[k]);
  }
  return 0;
}
