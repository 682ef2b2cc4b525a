// grad.hip -- vector calculus of stacked full-grid fields (cheb_grad_*, include/chebhip.h; field-major, row-major, all nodes: the
// layout of cheb_modal_*): gradient, divergence, curl, strain rate and Laplacian as SIGNED SWEEPS of the library's derivative kernels,
// and the pointwise invariants of a velocity-gradient tensor as one kernel of its own.
//
// Linear operators.  Every output array is a list of terms alpha * D_k in (or alpha * (D D)_k in): the first is stored (OUT_STORE),
// the later ones are accumulated into the same array (OUT_ACC), in the order the header writes them; alpha carries the sign, the 1/2
// of the strain and the direction's scale.  The schedule is by ROUNDS: round r holds the r-th term of every output, so the jobs of
// a round write different arrays and read only inputs (which may overlap no output): they are independent, and go to
// sweep_launch_multi in groups of at most 9 -- one launch where the 16-byte kernels take the group (plain stores, one matrix size
// class, 16-byte aligned fields), one launch per job otherwise.  Rounds follow each other on the stream, so an accumulate always finds
// its array's earlier terms.  Nothing depends on timing: the same call gives the same bits.  A first term may name an array `acc` of
// its own (cheb_grad_axpy_grad, the projection's out_k = u_k - s_k D_k phi): it is then added to acc instead of stored.
//
// Invariants.  k_grad_invariants reads the tensor G[v][c][k] (what cheb_grad_tensor writes) once and writes the selected fields; the
// diagonal entries are loaded only if a selected field needs them, the off-diagonal ones likewise.  d <= 3 keeps the d^2 entries of
// a node in registers; a larger d walks the pairs (c, k > c), two loads per pair.  No LDS, no atomics, no scratch.
#include "../../include/chebhip.h"
#include "sweep.h"
#include "ops.h"
#include "rowpass.h"
#include <map>
#include <new>
#include <utility>
#include <vector>

using namespace chebhip;

namespace {

constexpr int MD = 10;          // directions
constexpr int MAXF = 16;        // input fields of a call
constexpr int GROUP = 9;        // jobs of one sweep_launch_multi

constexpr unsigned NEED_DIAG = CHEB_INV_DIV | CHEB_INV_STRAIN2 | CHEB_INV_GAMMA | CHEB_INV_Q | CHEB_INV_NORM2;
constexpr unsigned NEED_OFF = CHEB_INV_VORT2 | CHEB_INV_STRAIN2 | CHEB_INV_GAMMA | CHEB_INV_Q | CHEB_INV_NORM2;
constexpr unsigned INV_ALL = NEED_DIAG | NEED_OFF;

template <class T> __device__ __forceinline__ T splat(double v);
template <> __device__ __forceinline__ double splat<double>(double v) { return v; }
template <> __device__ __forceinline__ d2 splat<d2>(double v) { return (d2){v, v}; }

// DC: the dimension compiled in (1..3), 0: `d` at run time.  T: double (one node per lane) or d2 (two nodes, 16-byte accesses; N even
// and both arrays 16-byte aligned).  npl = N / nodes per lane; total = nv * npl.
template <int DC, class T>
__global__ __launch_bounds__(256) void k_grad_invariants(int d, long N, long npl, long total, unsigned mask, int nsel,
                                                         const double *__restrict__ G, double *__restrict__ out) {
  constexpr int W = (int)(sizeof(T) / sizeof(double));
  const int dd = DC ? DC : d;
  const bool diag = (mask & NEED_DIAG) != 0, off = (mask & NEED_OFF) != 0;
  GS_LOOP(i, total) {
    const long v = i / npl, l = (i - v * npl) * W;
    const double *g = G + (size_t)v * dd * dd * N + l;
    T div = splat<T>(0.0), vort = splat<T>(0.0), sdiag = splat<T>(0.0), soff = splat<T>(0.0), norm = splat<T>(0.0);
    if constexpr (DC != 0) {
      T a[DC][DC];
#pragma unroll
      for (int c = 0; c < DC; c++)
#pragma unroll
        for (int k = 0; k < DC; k++)
          a[c][k] = (c == k ? diag : off) ? *reinterpret_cast<const T *>(g + (size_t)(c * DC + k) * N) : splat<T>(0.0);
#pragma unroll
      for (int c = 0; c < DC; c++) { div += a[c][c]; sdiag += a[c][c] * a[c][c]; }
#pragma unroll
      for (int c = 0; c < DC; c++)
#pragma unroll
        for (int k = c + 1; k < DC; k++) {
          const T w = a[k][c] - a[c][k], s = a[c][k] + a[k][c];
          vort += w * w; soff += s * s;
        }
#pragma unroll
      for (int c = 0; c < DC; c++)
#pragma unroll
        for (int k = 0; k < DC; k++) norm += a[c][k] * a[c][k];
    } else {
      for (int c = 0; c < dd; c++) {
        if (diag) {
          const T x = *reinterpret_cast<const T *>(g + (size_t)(c * dd + c) * N);
          div += x; sdiag += x * x; norm += x * x;
        }
        if (off)
          for (int k = c + 1; k < dd; k++) {
            const T p = *reinterpret_cast<const T *>(g + (size_t)(c * dd + k) * N);
            const T q = *reinterpret_cast<const T *>(g + (size_t)(k * dd + c) * N);
            const T w = q - p, s = p + q;
            vort += w * w; soff += s * s;
            norm += p * p; norm += q * q;
          }
      }
    }
    const T strain = sdiag + 0.5 * soff;
    double *o = out + (size_t)v * nsel * N + l;
    if (mask & CHEB_INV_DIV) { *reinterpret_cast<T *>(o) = div; o += N; }
    if (mask & CHEB_INV_VORT2) { *reinterpret_cast<T *>(o) = vort; o += N; }
    if (mask & CHEB_INV_STRAIN2) { *reinterpret_cast<T *>(o) = strain; o += N; }
    if (mask & CHEB_INV_GAMMA) { *reinterpret_cast<T *>(o) = 0.5 * strain; o += N; }
    if (mask & CHEB_INV_Q) { *reinterpret_cast<T *>(o) = 0.25 * vort - 0.5 * strain; o += N; }
    if (mask & CHEB_INV_NORM2) { *reinterpret_cast<T *>(o) = norm; o += N; }
  }
}

template <class T>
void launch_invariants(int d, long N, int nv, unsigned mask, int nsel, const double *G, double *out, hipStream_t st) {
  const long npl = N / (long)(sizeof(T) / sizeof(double)), total = (long)nv * npl;
  const dim3 grid(grid1d(total, 256, 4096)), block(256);
  switch (d) {
    case 1: hipLaunchKernelGGL((k_grad_invariants<1, T>), grid, block, 0, st, d, N, npl, total, mask, nsel, G, out); break;
    case 2: hipLaunchKernelGGL((k_grad_invariants<2, T>), grid, block, 0, st, d, N, npl, total, mask, nsel, G, out); break;
    case 3: hipLaunchKernelGGL((k_grad_invariants<3, T>), grid, block, 0, st, d, N, npl, total, mask, nsel, G, out); break;
    default: hipLaunchKernelGGL((k_grad_invariants<0, T>), grid, block, 0, st, d, N, npl, total, mask, nsel, G, out);
  }
}

// one term of one output array: out (+)= alpha * M_k in, M = D or D D
struct Term { const DiffMat *m; int k; const double *in; double alpha; const double *acc = nullptr; };

}  // namespace

struct cheb_grad {
  int d = 0;
  int n[MD] = {0};
  double scale[MD] = {0};
  unsigned inner[MD] = {0};
  long N = 0;
  int basis[MD] = {0};                // BASIS_CGL / BASIS_FOURIER per direction (cheb_grad_create_basis)
  std::map<std::pair<int, int>, DiffMat> D, DD;      // by (extent, basis); DD for 3 <= n <= 256 (Fourier: 2 <= n <= 256)
  const DiffMat *Dk(int k) const { return &D.at(std::make_pair(n[k], basis[k])); }
  const DiffMat &DDk(int k) const { return DD.at(std::make_pair(n[k], basis[k])); }
  bool two_sweeps = false;           // some direction has more than 256 points: the Laplacian needs `work`

  SweepParams job(const Term &t, double *out, bool acc, int nfields = 1) const {
    SweepParams sp = {};
    sp.ncols = (unsigned)((long)nfields * N / n[t.k]); sp.inner = inner[t.k];
    sp.in0 = t.in; sp.in_mode = IN_PLAIN;
    sp.alpha = t.alpha; sp.out = out;
    if (acc) { sp.out_mode = OUT_ACC; sp.acc = out; } else sp.out_mode = OUT_STORE;
    return sp;
  }
};

namespace {

// terms[o]: the terms of output array outs[o], every output with at least one.  Round r = the r-th term of every output that has one.
int run_rounds(const cheb_grad *h, const std::vector<std::vector<Term>> &terms, const std::vector<double *> &outs, hipStream_t st) {
  size_t rounds = 0;
  for (const auto &t : terms) rounds = std::max(rounds, t.size());
  const DiffMat *m[GROUP]; SweepParams sp[GROUP];
  for (size_t r = 0; r < rounds; r++) {
    int n = 0;
    for (size_t o = 0; o < terms.size(); o++) {
      if (r >= terms[o].size()) continue;
      m[n] = terms[o][r].m; sp[n] = h->job(terms[o][r], outs[o], r > 0);
      if (r == 0 && terms[o][0].acc) { sp[n].out_mode = OUT_ACC; sp[n].acc = terms[o][0].acc; }
      n++;
      if (n == GROUP) { HIP_TRY(sweep_launch_multi(n, m, sp, st)); n = 0; }
    }
    if (n) HIP_TRY(sweep_launch_multi(n, m, sp, st));
  }
  return 0;
}

int check_call(const cheb_grad *h, int nfields_in, const char *what) {
  if (nfields_in < 1 || nfields_in > MAXF) return chebhip_fail(CHEBHIP_ERR_ARG, "%s: %d input fields, must be in 1..16", what, nfields_in);
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "%s: NULL handle", what);
  return 0;
}

int check_arrays(const cheb_grad *h, const char *what, const double *in, long nin, const double *out, long nout) {
  if (!in || !out) return chebhip_fail(CHEBHIP_ERR_ARG, "%s: NULL array", what);
  if (nin * h->N >= 0x80000000L || nout * h->N >= 0x80000000L) return chebhip_fail(CHEBHIP_ERR_DIMS, "%s: 2^31 values or more", what);
  if (overlap(in, nin * h->N, out, nout * h->N)) return chebhip_fail(CHEBHIP_ERR_ARG, "%s: the output must not overlap the input", what);
  return 0;
}

}  // namespace

extern "C" int cheb_grad_destroy(cheb_grad *h) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  for (auto &kv : h->D) diffmat_destroy(&kv.second);
  for (auto &kv : h->DD) diffmat_destroy(&kv.second);
  delete h;
  return 0;
}

// basis[k]: BASIS_CGL or BASIS_FOURIER (a periodic direction of 2 <= n <= 256 nodes x_j = -1 + 2 j / n: D_F and D_F D_F of diffmat.cpp
// through diffmat_from_dense); null: CGL everywhere, which is cheb_grad_create
static int grad_create(int d, const int *dims, const double *scale, const int *basis, cheb_grad **out) {
  if (!out) return chebhip_fail(CHEBHIP_ERR_ARG, "out is NULL");
  *out = nullptr;
  int rc;
  long N = 0;
  if ((rc = check_field_grid(d, dims, basis, 1, &N, nullptr))) return rc;      // (the handle has no field count: calls bring theirs)
  for (int k = 0; k < d; k++)
    if (scale && !(scale[k] == scale[k] && scale[k] - scale[k] == 0.0)) return chebhip_fail(CHEBHIP_ERR_ARG, "scale[%d] is not finite", k);
  if ((rc = require_device())) return rc;
  cheb_grad *h = new (std::nothrow) cheb_grad;
  if (!h) return chebhip_fail(CHEBHIP_ERR_MEMORY, "out of host memory");
  h->d = d; h->N = N;
  unsigned in = 1;
  for (int k = d - 1; k >= 0; k--) { h->n[k] = dims[k]; h->scale[k] = scale ? scale[k] : 1.0; h->inner[k] = in; in *= (unsigned)dims[k]; }
  for (int k = 0; k < d; k++) {
    const int n = dims[k], b = h->basis[k] = basis ? basis[k] : BASIS_CGL;
    const std::pair<int, int> key(n, b);
    if (n > 256) h->two_sweeps = true;
    if (b == BASIS_FOURIER) {
      if (!h->D.count(key)) { DiffMat m; HIP_TRY_OR(diffmat_create_fourier(n, 1, &m), cheb_grad_destroy(h)); h->D[key] = m; }
      if (!h->DD.count(key)) { DiffMat m; HIP_TRY_OR(diffmat_create_fourier(n, 2, &m), cheb_grad_destroy(h)); h->DD[key] = m; }
      continue;
    }
    if (!h->D.count(key)) { DiffMat m; HIP_TRY_OR(diffmat_create(n, &m), cheb_grad_destroy(h)); h->D[key] = m; }
    if (n >= 3 && n <= 256 && !h->DD.count(key)) { DiffMat m; HIP_TRY_OR(diffmat_create_dd(n, &m), cheb_grad_destroy(h)); h->DD[key] = m; }
  }
  *out = h;
  return 0;
}

extern "C" int cheb_grad_create(int d, const int *dims, const double *scale, cheb_grad **out) { return grad_create(d, dims, scale, nullptr, out); }

extern "C" int cheb_grad_create_basis(int d, const int *dims, const double *scale, const int *basis, cheb_grad **out) {
  if (out) *out = nullptr;
  if (!basis) return chebhip_fail(CHEBHIP_ERR_ARG, "basis is NULL");
  return grad_create(d, dims, scale, basis, out);
}

extern "C" long cheb_grad_size(const cheb_grad *h) { return h ? h->N : -1; }

extern "C" long cheb_grad_work_size(const cheb_grad *h, int nfields) {
  if (!h || nfields < 1 || nfields > MAXF) return -1;
  return h->two_sweeps ? (long)nfields * h->N : 0;
}

// out[f * d + k] = s_k d_k s[f]
extern "C" int cheb_grad_grad(cheb_grad *h, int nfields, const double *s_dev, double *out_dev, void *stream) {
  int rc;
  if ((rc = check_call(h, nfields, "grad"))) return rc;
  if ((rc = check_arrays(h, "grad", s_dev, nfields, out_dev, (long)nfields * h->d))) return rc;
  const int d = h->d; const long N = h->N;
  std::vector<std::vector<Term>> terms; std::vector<double *> outs;
  for (int f = 0; f < nfields; f++)
    for (int k = 0; k < d; k++) {
      terms.push_back({Term{h->Dk(k), k, s_dev + (size_t)f * N, h->scale[k]}});
      outs.push_back(out_dev + (size_t)(f * d + k) * N);
    }
  return run_rounds(h, terms, outs, (hipStream_t)stream);
}

// G[v][c][k] = s_k d_k u[v][c]: the gradient of the nv * d scalars
extern "C" int cheb_grad_tensor(cheb_grad *h, int nvec, const double *u_dev, double *G_dev, void *stream) {
  int rc;
  if ((rc = check_call(h, h ? nvec * h->d : nvec, "tensor"))) return rc;
  if (nvec < 1) return chebhip_fail(CHEBHIP_ERR_ARG, "tensor: %d vectors", nvec);
  return cheb_grad_grad(h, nvec * h->d, u_dev, G_dev, stream);
}

// out[v] = ((s_0 d_0 u[v][0]) + s_1 d_1 u[v][1]) + ...
extern "C" int cheb_grad_div(cheb_grad *h, int nvec, const double *u_dev, double *out_dev, void *stream) {
  int rc;
  if (nvec < 1) return chebhip_fail(CHEBHIP_ERR_ARG, "div: %d vectors", nvec);
  if ((rc = check_call(h, h ? nvec * h->d : nvec, "div"))) return rc;
  if ((rc = check_arrays(h, "div", u_dev, (long)nvec * h->d, out_dev, nvec))) return rc;
  const int d = h->d; const long N = h->N;
  std::vector<std::vector<Term>> terms(nvec); std::vector<double *> outs(nvec);
  for (int v = 0; v < nvec; v++) {
    outs[v] = out_dev + (size_t)v * N;
    for (int k = 0; k < d; k++) terms[v].push_back(Term{h->Dk(k), k, u_dev + (size_t)(v * d + k) * N, h->scale[k]});
  }
  return run_rounds(h, terms, outs, (hipStream_t)stream);
}

// out[v * d + k] = u[v * d + k] + alpha s_k d_k s[v]: one accumulating sweep per output (csrc/ops.h; project.hip).  out may be u,
// s may overlap neither; the caller has checked the arrays.
int cheb_grad_axpy_grad(cheb_grad *h, int nvec, double alpha, const double *s_dev, const double *u_dev, double *out_dev, void *stream) {
  int rc;
  if (nvec < 1) return chebhip_fail(CHEBHIP_ERR_ARG, "axpy_grad: %d vectors", nvec);
  if ((rc = check_call(h, h ? nvec * h->d : nvec, "axpy_grad"))) return rc;
  const int d = h->d; const long N = h->N;
  std::vector<std::vector<Term>> terms; std::vector<double *> outs;
  for (int v = 0; v < nvec; v++)
    for (int k = 0; k < d; k++) {
      terms.push_back({Term{h->Dk(k), k, s_dev + (size_t)v * N, alpha * h->scale[k], u_dev + (size_t)(v * d + k) * N}});
      outs.push_back(out_dev + (size_t)(v * d + k) * N);
    }
  return run_rounds(h, terms, outs, (hipStream_t)stream);
}

// d = 3: w_0 = d_1 u_2 - d_2 u_1, w_1 = d_2 u_0 - d_0 u_2, w_2 = d_0 u_1 - d_1 u_0; d = 2: the one field d_0 u_1 - d_1 u_0
extern "C" int cheb_grad_curl(cheb_grad *h, int nvec, const double *u_dev, double *out_dev, void *stream) {
  int rc;
  if (nvec < 1) return chebhip_fail(CHEBHIP_ERR_ARG, "curl: %d vectors", nvec);
  if ((rc = check_call(h, h ? nvec * h->d : nvec, "curl"))) return rc;
  if (h->d != 2 && h->d != 3) return chebhip_fail(CHEBHIP_ERR_ARG, "curl: d = %d, defined for 2 and 3", h->d);
  const int d = h->d, no = d == 3 ? 3 : 1; const long N = h->N;
  if ((rc = check_arrays(h, "curl", u_dev, (long)nvec * d, out_dev, (long)nvec * no))) return rc;
  std::vector<std::vector<Term>> terms; std::vector<double *> outs;
  auto term = [&](int v, int k, int c, double sign) { return Term{h->Dk(k), k, u_dev + (size_t)(v * d + c) * N, sign * h->scale[k]}; };
  for (int v = 0; v < nvec; v++) {
    if (d == 2) { terms.push_back({term(v, 0, 1, 1.0), term(v, 1, 0, -1.0)}); outs.push_back(out_dev + (size_t)v * N); continue; }
    for (int i = 0; i < 3; i++) {
      const int a = (i + 1) % 3, b = (i + 2) % 3;                       // w_i = d_a u_b - d_b u_a
      terms.push_back({term(v, a, b, 1.0), term(v, b, a, -1.0)});
      outs.push_back(out_dev + (size_t)(v * 3 + i) * N);
    }
  }
  return run_rounds(h, terms, outs, (hipStream_t)stream);
}

// per vector the d (d + 1) / 2 fields (0,0), (0,1), .., (d-1,d-1): S_cc = s_c d_c u_c, S_ck = 1/2 s_k d_k u_c + 1/2 s_c d_c u_k
extern "C" int cheb_grad_strain(cheb_grad *h, int nvec, const double *u_dev, double *out_dev, void *stream) {
  int rc;
  if (nvec < 1) return chebhip_fail(CHEBHIP_ERR_ARG, "strain: %d vectors", nvec);
  if ((rc = check_call(h, h ? nvec * h->d : nvec, "strain"))) return rc;
  const int d = h->d, ns = d * (d + 1) / 2; const long N = h->N;
  if ((rc = check_arrays(h, "strain", u_dev, (long)nvec * d, out_dev, (long)nvec * ns))) return rc;
  std::vector<std::vector<Term>> terms; std::vector<double *> outs;
  for (int v = 0; v < nvec; v++) {
    int o = 0;
    const double *u = u_dev + (size_t)v * d * N;
    for (int c = 0; c < d; c++)
      for (int k = c; k < d; k++, o++) {
        if (k == c) terms.push_back({Term{h->Dk(c), c, u + (size_t)c * N, h->scale[c]}});
        else terms.push_back({Term{h->Dk(k), k, u + (size_t)c * N, 0.5 * h->scale[k]},
                              Term{h->Dk(c), c, u + (size_t)k * N, 0.5 * h->scale[c]}});
        outs.push_back(out_dev + (size_t)(v * ns + o) * N);
      }
  }
  return run_rounds(h, terms, outs, (hipStream_t)stream);
}

// out[f] = sum_k s_k^2 d_k^2 s[f], directions ascending; the nfields fields are one tensor with one more outer direction, so a
// direction is one sweep over all of them (3 <= n_k <= 256: D D) or two (n_k > 256: D into `work`, D of `work`); n_k = 2 adds nothing
extern "C" int cheb_grad_laplacian(cheb_grad *h, int nfields, const double *s_dev, double *work_dev, double *out_dev, void *stream) {
  int rc;
  if ((rc = check_call(h, nfields, "laplacian"))) return rc;
  if ((rc = check_arrays(h, "laplacian", s_dev, nfields, out_dev, nfields))) return rc;
  const long total = (long)nfields * h->N;
  if (h->two_sweeps) {
    if (!work_dev) return chebhip_fail(CHEBHIP_ERR_ARG, "laplacian: a direction of more than 256 points needs the work array");
    if (overlap(work_dev, total, s_dev, total) || overlap(work_dev, total, out_dev, total))
      return chebhip_fail(CHEBHIP_ERR_ARG, "laplacian: the work array must not overlap the input or the output");
  }
  hipStream_t st = (hipStream_t)stream;
  bool first = true;
  for (int k = 0; k < h->d; k++) {
    const int n = h->n[k];
    const double a = h->scale[k] * h->scale[k];
    if (n == 2) continue;
    if (n <= 256) {
      HIP_TRY(sweep_launch(h->DDk(k), h->job(Term{nullptr, k, s_dev, a}, out_dev, !first, nfields), st));
    } else {
      HIP_TRY(sweep_launch(*h->Dk(k), h->job(Term{nullptr, k, s_dev, 1.0}, work_dev, false, nfields), st));
      HIP_TRY(sweep_launch(*h->Dk(k), h->job(Term{nullptr, k, work_dev, a}, out_dev, !first, nfields), st));
    }
    first = false;
  }
  if (first) HIP_TRY(hipMemsetAsync(out_dev, 0, (size_t)total * sizeof(double), st));       // every extent is 2: D D = 0
  return 0;
}

extern "C" int cheb_grad_invariants(cheb_grad *h, int nvec, const double *G_dev, unsigned mask, double *out_dev, void *stream) {
  int rc;
  if ((rc = check_call(h, nvec, "invariants"))) return rc;
  if (mask == 0 || (mask & ~INV_ALL)) return chebhip_fail(CHEBHIP_ERR_ARG, "invariants: mask 0x%x selects nothing or an unknown field", mask);
  const int nsel = __builtin_popcount(mask);
  if ((rc = check_arrays(h, "invariants", G_dev, (long)nvec * h->d * h->d, out_dev, (long)nvec * nsel))) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (h->N & 1) == 0 && (((size_t)G_dev | (size_t)out_dev) & 15) == 0;
  if (vec) launch_invariants<d2>(h->d, h->N, nvec, mask, nsel, G_dev, out_dev, st);
  else launch_invariants<double>(h->d, h->N, nvec, mask, nsel, G_dev, out_dev, st);
  sweep_note_launch();
  HIP_TRY(hipGetLastError());
  return 0;
}
