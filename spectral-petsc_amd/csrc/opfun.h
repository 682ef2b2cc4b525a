// opfun.h -- what the handle of ChebOpFun (precond.hip, next to the solver whose lines it borrows) needs of opfun.hip: the term table
// in the form the mixing kernel takes by value, and the kernel's launch.
#pragma once
#include "../../include/chebhip.h"
#include <hip/hip_runtime.h>

namespace chebhip {

constexpr int OPFUN_MAX_TERMS = 32, OPFUN_MAX_FIELDS = 16;

// The terms sorted by output (stable: table order within an output), the distinct (kind, tau, par) numbered once.  888 bytes.
struct OpfunTable {
  double coef[OPFUN_MAX_TERMS];                        // per sorted term
  double tau[OPFUN_MAX_TERMS], par[OPFUN_MAX_TERMS];   // per distinct weight
  unsigned char kind[OPFUN_MAX_TERMS];                 // per distinct weight
  unsigned char in[OPFUN_MAX_TERMS], slot[OPFUN_MAX_TERMS];   // per sorted term: input field, weight number
  unsigned char first[OPFUN_MAX_FIELDS + 1];           // output o owns the sorted terms first[o] .. first[o + 1] - 1
  unsigned char nweights, nin, nout;
};

// checks every term (CHEBHIP_ERR_ARG otherwise) and fills *tb; host only
int opfun_build_table(int nin, int nout, int nterms, const cheb_opfun_term *terms, OpfunTable *tb);
int opfun_check_weight(int kind, double tau, double par);
// y (nout fields of G values) from x (nin fields, another array) in mode space: M[k] interior extents, lam[k] device eigenvalues
// (lam[0] carries sigma)
int opfun_mix_launch(const OpfunTable &tb, int d, const int *M, long G, const double *const *lam, const double *x, double *y, hipStream_t st);

}  // namespace chebhip
