// project.hip -- the projection of stacked full-grid velocity fields onto discretely divergence-free ones on a box
// (cheb_project_*, include/chebhip.h): out_k = u_k - s_k d_k phi with phi the solution of the collocation problem
//     sum_k s_k^2 (D D)_k phi = sum_k s_k d_k u_k  at the interior nodes,
//     +- s_k d_k phi = +- u_k - flux  at the nodes of a wall,   phi = 0  at the nodes of an open face,
// a boundary node taking the condition of the highest direction in which it is an end node (the edge rule of DESIGN 10c).
//
// A call is four steps on one stream, none of them a new sweep or solver kernel: the divergence (cheb_grad_div, into phi as
// scratch), k_project_rhs (the one kernel of this file: the solver's interior right-hand side f = -div u and its compact boundary
// data g from the divergence, u and the flux), cheb_helmholtz_solve_bc of a box handle (sigma = 0; (0, 1) ends at walls, (1, 0) at
// open faces), and one accumulating sweep per output component (cheb_grad_axpy_grad: out_k = u_k + (-s_k) D_k phi).
//
// A periodic direction (cheb_project_create_basis) has no faces: cheb_grad and the solver are their _basis handles, the
// unknowns are the nodes interior in every WALL direction (the solver's geometry) and the tables below follow that.  With every
// direction periodic there is no boundary node, no g and no face table.
//
// Variable density (cheb_project_create_variable): out_k = u_k - kappa s_k d_k phi with kappa = 1 / rho one full-grid
// field, phi from  sum_k s_k^2 d_k(kappa d_k phi) = div u  with  kappa s_k dphi/dnu = +- u_k - flux  on walls.  The handle owns a
// cheb_varhelm (c = 0, nvec fields) in place of the direct solve: k_project_rhs divides a wall node's data by kappa there (the
// operator's faces carry no kappa), cheb_varhelm_solve_deflated finds the unknowns (kept on the handle: the next call's guess where
// it asks for one) and extends them into phi, and the correction is the gradient of phi into d work grids per vector
// (cheb_grad_grad), k_project_wall_grad (the normal derivative at a wall node is the datum that defines phi's end value there)
// and one pointwise pass, k_project_correct.
//
// k_project_rhs: grid-stride over the nodes, one node per lane, the vectors along the grid's second dimension.  The handle's node table (ChebLayout's: m >= 0 the
// number among the interior nodes, -1 - b on the boundary) sends a node's value to f or g; the face table gives a boundary node's
// (direction, end) as 2 k + end.  Values are moved and negated, a flux is one subtraction; the field side is read coalesced.  No
// LDS, no atomics, no scratch.
#include "../../include/chebhip.h"
#include "sweep.h"
#include "ops.h"
#include <cmath>
#include <new>
#include <vector>

using namespace chebhip;

namespace {

constexpr int MD = 10;

// blockIdx.y: the vector.  openf: bit 2 k + end set = that face is open (g = 0).  VAR: a wall node's value is divided by kappa there
template <bool VAR>
__global__ __launch_bounds__(256) void k_project_rhs(long N, long G, long NB, int d, unsigned openf, const int *__restrict__ map,
                                                     const unsigned char *__restrict__ face, const double *__restrict__ div,
                                                     const double *__restrict__ u, const double *__restrict__ flux, const double *__restrict__ kappa,
                                                     double *__restrict__ f, double *__restrict__ g) {
  const long v = blockIdx.y;
  GS_LOOP(l, N) {
    const int m = map[l];
    if (m >= 0) { f[v * G + m] = -div[v * N + l]; continue; }
    const long b = -1 - (long)m;
    const int fc = face[b];
    double val = 0.0;
    if (!((openf >> fc) & 1u)) {
      const double un = u[(size_t)(v * d + (fc >> 1)) * N + l];
      val = (fc & 1) ? -un : un;
      if (flux) val -= flux[v * NB + b];
      if constexpr (VAR) val /= kappa[l];
    }
    g[v * NB + b] = val;
  }
}

// The normal derivative of phi at the nodes that take a wall's condition, from that condition: phi's end value there is DEFINED by
// +- s_k d_k phi = g (the row the extension solves), so gw[v][k] = +-g at the node, where the sweep's value is the same number
// carrying the rounding of the end value times the row's corner entry (2 n^2 + 1) / 6.  With it the normal velocity of the result
// is u_k - kappa ((+-u_k - flux) / kappa): flux to three roundings.  blockIdx.y: the vector; nodes of open faces are left alone.
__global__ __launch_bounds__(256) void k_project_wall_grad(long N, long NB, int d, unsigned openf, const int *__restrict__ map,
                                                           const unsigned char *__restrict__ face, const double *__restrict__ g, double *__restrict__ gw) {
  const long v = blockIdx.y;
  GS_LOOP(l, N) {
    const int m = map[l];
    if (m >= 0) continue;
    const long b = -1 - (long)m;
    const int fc = face[b];
    if ((openf >> fc) & 1u) continue;
    const double gv = g[v * NB + b];
    gw[(size_t)(v * d + (fc >> 1)) * N + l] = (fc & 1) ? -gv : gv;       // outward: + s_k d_k at index 0, - s_k d_k at the last
  }
}

// The variable-density correction: out[c] = u[c] - kappa * gw[c] over the nvec * d components c = blockIdx.y, gw = s_k d_k phi.
// out may be u (a lane reads and writes the same elements).  W = 2: N even, every array 16-byte aligned.
typedef double pj2 __attribute__((ext_vector_type(2)));
template <class T>
__global__ __launch_bounds__(256) void k_project_correct(long N, const double *__restrict__ kappa, const double *__restrict__ gw, const double *u, double *out) {
  constexpr long W = (long)(sizeof(T) / sizeof(double));
  const size_t c = (size_t)blockIdx.y * N;
  GS_LOOP(i, N / W) {
    const long l = i * W;
    *reinterpret_cast<T *>(out + c + l) = *reinterpret_cast<const T *>(u + c + l) - *reinterpret_cast<const T *>(kappa + l) * *reinterpret_cast<const T *>(gw + c + l);
  }
}

// basis: null (walls everywhere) or one CHEB_BASIS_* per direction.  A wall direction has 3 .. 258 points and dims - 2 unknowns, a
// periodic one 2 .. 256 points, all of them unknowns (the ranges of cheb_helmholtz_create_basis).  G: the unknown nodes.
int check_grid(int d, const int *dims, const int *basis, long *N_out, long *G_out) {
  if (!dims || d < 1 || d > MD) return chebhip_fail(CHEBHIP_ERR_DIMS, "d = %d must be in 1..10", d);
  long N = 1, G = 1;
  for (int k = 0; k < d; k++) {
    if (basis && basis[k] != CHEB_BASIS_CGL && basis[k] != CHEB_BASIS_FOURIER)
      return chebhip_fail(CHEBHIP_ERR_ARG, "basis[%d] = %d is neither 0 (CGL) nor 1 (Fourier)", k, basis[k]);
    if (basis && basis[k] == CHEB_BASIS_FOURIER) {
      if (dims[k] < 2) return chebhip_fail(CHEBHIP_ERR_SIZE, "dims[%d] = %d: a periodic direction needs at least 2 points", k, dims[k]);
      if (dims[k] > 256) return chebhip_fail(CHEBHIP_ERR_ARG, "dims[%d] = %d: a periodic direction supports at most 256 points", k, dims[k]);
      N *= dims[k]; G *= dims[k];
    } else {
      if (dims[k] < 3) return chebhip_fail(CHEBHIP_ERR_SIZE, "dims[%d] = %d but must be >= 3: a line needs an interior node", k, dims[k]);
      if (dims[k] > 258) return chebhip_fail(CHEBHIP_ERR_ARG, "dims[%d] = %d: the direct solve supports at most 258 points per line", k, dims[k]);
      N *= dims[k]; G *= dims[k] - 2;
    }
    if (N >= 0x80000000L) return chebhip_fail(CHEBHIP_ERR_DIMS, "2^31 nodes or more");
  }
  *N_out = N; *G_out = G;
  return 0;
}

// one node walk for both tables (either may be null), in the solver's geometry (cheb_helmholtz_create_basis): a node is an unknown if
// it is interior in every wall direction -- map[l] = its number among the unknowns, row-major -- and a boundary node otherwise:
// map[l] = -1 - b, face[b] = 2 k + end of the highest WALL direction in which it is an end node.  A periodic direction has no ends.
// basis null: map as cheb_layout_map_host.
void walk(int d, const int *dims, const int *basis, int *map, int *face) {
  BoxGrid box;
  box.set_box(d, dims, 0, dims[0]);
  auto end = [&](const int *ind, int k) { return !(basis && basis[k] == CHEB_BASIS_FOURIER) && (ind[k] == 0 || ind[k] == dims[k] - 1); };
  int g = 0, b = 0;
  box.for_each_node([&](long l, const int *ind, bool) {
    int k = d - 1;
    while (k >= 0 && !end(ind, k)) k--;
    if (k < 0) { if (map) map[l] = g; g++; return; }
    if (face) face[b] = 2 * k + (ind[k] != 0);
    if (map) map[l] = -1 - b;
    b++;
  });
}

}  // namespace

struct cheb_project {
  int d = 0, nvec = 0;
  long N = 0, G = 0;
  unsigned open = 0;                 // bit 2 k + end
  cheb_grad *grad = nullptr;
  cheb_helmholtz *hz = nullptr;
  int *map = nullptr;                // device [N]
  unsigned char *face = nullptr;     // device [N - G]
  double *f = nullptr, *g = nullptr; // device [nvec * G], [nvec * (N - G)]
  // cheb_project_create_variable: the solver in place of hz, the unknowns of the last solve, the gradient of phi
  cheb_varhelm *vh = nullptr;
  double *x = nullptr, *gw = nullptr; // device [nvec * G], [nvec * d * N]
  bool have_x = false;
};

extern "C" int cheb_project_destroy(cheb_project *h) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (h->grad) cheb_grad_destroy(h->grad);
  if (h->hz) cheb_helmholtz_destroy(h->hz);
  if (h->vh) cheb_varhelm_destroy(h->vh);
  if (h->x) (void)hipFree(h->x);
  if (h->gw) (void)hipFree(h->gw);
  if (h->map) (void)hipFree(h->map);
  if (h->face) (void)hipFree(h->face);
  if (h->f) (void)hipFree(h->f);
  if (h->g) (void)hipFree(h->g);
  delete h;
  return 0;
}

extern "C" int cheb_project_faces_host(int d, const int *dims, int *face) {
  int rc; long N, G;
  if ((rc = check_grid(d, dims, nullptr, &N, &G))) return rc;
  if (!face) return chebhip_fail(CHEBHIP_ERR_ARG, "face is NULL");
  walk(d, dims, nullptr, nullptr, face);
  return 0;
}

extern "C" int cheb_project_faces_basis_host(int d, const int *dims, const int *basis, int *face) {
  if (!basis) return chebhip_fail(CHEBHIP_ERR_ARG, "basis is NULL");
  int rc; long N, G;
  if ((rc = check_grid(d, dims, basis, &N, &G))) return rc;
  if (!face && N != G) return chebhip_fail(CHEBHIP_ERR_ARG, "face is NULL");
  walk(d, dims, basis, nullptr, face);
  return 0;
}

// Everything of a handle but its solver: the checks, cheb_grad, the node tables, f and g.  bc: the solver's 4 d end coefficients
// ((0, 1) at walls, (1, 0) at open faces).  basis null: cheb_project_create, the handles and the calls it has always made.
static int project_create_common(int d, const int *dims, const int *basis, const int *faces, const double *scale, int nvec, double *bc, cheb_project **out) {
  int rc; long N, G;
  if ((rc = check_grid(d, dims, basis, &N, &G))) return rc;
  if (nvec < 1 || (long)nvec * d > 16) return chebhip_fail(CHEBHIP_ERR_ARG, "nvec = %d: nvec * d must be in 1..16", nvec);
  if ((long)nvec * d * N >= 0x80000000L) return chebhip_fail(CHEBHIP_ERR_DIMS, "2^31 values or more");
  unsigned open = 0;
  for (int k = 0; k < d; k++) {
    if (scale && (!std::isfinite(scale[k]) || !(scale[k] > 0.0))) return chebhip_fail(CHEBHIP_ERR_ARG, "scale[%d] = %g must be finite and > 0", k, scale[k]);
    const bool fourier = basis && basis[k] == CHEB_BASIS_FOURIER;          // (no faces: its codes are not read)
    for (int e = 0; e < 2; e++) {
      const int kind = faces && !fourier ? faces[2 * k + e] : CHEB_FACE_WALL;
      if (kind != CHEB_FACE_WALL && kind != CHEB_FACE_OPEN) return chebhip_fail(CHEBHIP_ERR_ARG, "faces[%d] = %d: CHEB_FACE_WALL or CHEB_FACE_OPEN", 2 * k + e, kind);
      if (kind == CHEB_FACE_OPEN) open |= 1u << (2 * k + e);
      bc[4 * k + 2 * e] = kind == CHEB_FACE_OPEN ? 1.0 : 0.0;         // open: phi = 0; wall: s_k dphi/dnu = g
      bc[4 * k + 2 * e + 1] = kind == CHEB_FACE_OPEN ? 0.0 : 1.0;
    }
  }
  if ((rc = require_device())) return rc;
  cheb_project *h = new (std::nothrow) cheb_project;
  if (!h) return chebhip_fail(CHEBHIP_ERR_MEMORY, "out of host memory");
  h->d = d; h->nvec = nvec; h->N = N; h->G = G; h->open = open;
  rc = basis ? cheb_grad_create_basis(d, dims, scale, basis, &h->grad) : cheb_grad_create(d, dims, scale, &h->grad);
  if (rc) {
    cheb_project_destroy(h);
    return rc;
  }
  const long NB = N - G;                     // 0 with every direction periodic: no face table, no g
  std::vector<int> map((size_t)N), face((size_t)NB);
  walk(d, dims, basis, map.data(), face.data());
  std::vector<unsigned char> fc(face.begin(), face.end());
  HIP_TRY_MEM_OR(hipMalloc((void **)&h->map, (size_t)N * sizeof(int)), cheb_project_destroy(h));
  HIP_TRY_MEM_OR(hipMalloc((void **)&h->f, (size_t)nvec * G * sizeof(double)), cheb_project_destroy(h));
  HIP_TRY_OR(hipMemcpy(h->map, map.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice), cheb_project_destroy(h));
  if (NB) {
    HIP_TRY_MEM_OR(hipMalloc((void **)&h->face, (size_t)NB), cheb_project_destroy(h));
    HIP_TRY_MEM_OR(hipMalloc((void **)&h->g, (size_t)nvec * NB * sizeof(double)), cheb_project_destroy(h));
    HIP_TRY_OR(hipMemcpy(h->face, fc.data(), (size_t)NB, hipMemcpyHostToDevice), cheb_project_destroy(h));
  }
  *out = h;
  return 0;
}

static int project_create(int d, const int *dims, const int *basis, const int *faces, const double *scale, int nvec, cheb_project **out) {
  if (!out) return chebhip_fail(CHEBHIP_ERR_ARG, "out is NULL");
  *out = nullptr;
  double bc[4 * MD];
  cheb_project *h = nullptr;
  int rc = project_create_common(d, dims, basis, faces, scale, nvec, bc, &h);
  if (rc) return rc;
  rc = basis ? cheb_helmholtz_create_basis(d, dims, basis, bc, scale, 0.0, nvec, &h->hz) : cheb_helmholtz_create_box(d, dims, bc, scale, 0.0, nvec, &h->hz);
  if (rc) {
    cheb_project_destroy(h);
    return rc;
  }
  *out = h;
  return 0;
}

extern "C" int cheb_project_create(int d, const int *dims, const int *faces, const double *scale, int nvec, cheb_project **out) {
  return project_create(d, dims, nullptr, faces, scale, nvec, out);
}

extern "C" int cheb_project_create_basis(int d, const int *dims, const int *basis, const int *faces, const double *scale, int nvec, cheb_project **out) {
  if (out) *out = nullptr;
  if (!basis) return chebhip_fail(CHEBHIP_ERR_ARG, "basis is NULL");
  return project_create(d, dims, basis, faces, scale, nvec, out);
}

// basis may be null (walls and open faces only)
extern "C" int cheb_project_create_variable(int d, const int *dims, const int *basis, const int *faces, const double *scale, int nvec, cheb_project **out) {
  if (!out) return chebhip_fail(CHEBHIP_ERR_ARG, "out is NULL");
  *out = nullptr;
  double bc[4 * MD];
  cheb_project *h = nullptr;
  int rc = project_create_common(d, dims, basis, faces, scale, nvec, bc, &h);
  if (rc) return rc;
  if ((rc = cheb_varhelm_create(d, dims, basis, bc, scale, nvec, &h->vh))) {
    cheb_project_destroy(h);
    return rc;
  }
  HIP_TRY_MEM_OR(hipMalloc((void **)&h->x, (size_t)nvec * (h->G ? h->G : 1) * sizeof(double)), cheb_project_destroy(h));
  HIP_TRY_MEM_OR(hipMalloc((void **)&h->gw, (size_t)nvec * d * h->N * sizeof(double)), cheb_project_destroy(h));
  *out = h;
  return 0;
}

extern "C" long cheb_project_size(const cheb_project *h, int which) {
  if (!h || which < 0 || which > 2) return -1;
  return which == 0 ? h->N : which == 1 ? h->G : h->N - h->G;
}

// (a variable-density handle: as its faces make it -- c = 0 always -- whether or not the density has been set)
extern "C" int cheb_project_singular(const cheb_project *h) {
  if (!h) return -1;
  if (h->hz) return cheb_helmholtz_singular(h->hz);
  return h->open == 0 ? 1 : 0;
}
extern "C" cheb_varhelm *cheb_project_varhelm(const cheb_project *h) { return h ? h->vh : nullptr; }

// the argument checks of apply and apply_variable
static int project_check(const cheb_project *h, const double *u_dev, const double *flux_dev, const double *phi_dev, const double *out_dev) {
  if (!u_dev || !phi_dev || !out_dev) return chebhip_fail(CHEBHIP_ERR_ARG, "project: NULL array");
  const long N = h->N, G = h->G, NB = N - G, nu = (long)h->nvec * h->d * N, np = (long)h->nvec * N, nb = (long)h->nvec * NB;
  if (flux_dev && NB == 0) return chebhip_fail(CHEBHIP_ERR_ARG, "project: flux given, but every direction is periodic: there is no wall to prescribe it on");
  if (out_dev != u_dev && overlap(out_dev, nu, u_dev, nu)) return chebhip_fail(CHEBHIP_ERR_ARG, "project: out is u or does not overlap it");
  if (overlap(phi_dev, np, u_dev, nu) || overlap(phi_dev, np, out_dev, nu)) return chebhip_fail(CHEBHIP_ERR_ARG, "project: phi must not overlap u or out");
  if (flux_dev && (overlap(flux_dev, nb, u_dev, nu) || overlap(flux_dev, nb, out_dev, nu) || overlap(flux_dev, nb, phi_dev, np)))
    return chebhip_fail(CHEBHIP_ERR_ARG, "project: flux must not overlap u, out or phi");
  return 0;
}

extern "C" int cheb_project_apply(cheb_project *h, const double *u_dev, const double *flux_dev, double *phi_dev, double *out_dev, void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "project: NULL handle");
  if (!h->hz) return chebhip_fail(CHEBHIP_ERR_ARG, "project: a variable-density handle projects with cheb_project_apply_variable");
  int rc;
  if ((rc = project_check(h, u_dev, flux_dev, phi_dev, out_dev))) return rc;
  const long N = h->N, G = h->G, NB = N - G;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = cheb_grad_div(h->grad, h->nvec, u_dev, phi_dev, stream))) return rc;
  hipLaunchKernelGGL(k_project_rhs<false>, dim3(grid1d(N, 256, 4096), (unsigned)h->nvec), dim3(256), 0, st, N, G, NB, h->d, h->open, h->map, h->face, phi_dev, u_dev,
                     flux_dev, (const double *)nullptr, h->f, h->g);
  sweep_note_launch();
  HIP_TRY(hipGetLastError());
  // (every direction periodic: g and the face table are null, no node reads them, and the solve takes no boundary data)
  if ((rc = cheb_helmholtz_solve_bc(h->hz, h->f, h->g, phi_dev, stream))) return rc;
  return cheb_grad_axpy_grad(h->grad, h->nvec, -1.0, phi_dev, u_dev, out_dev, stream);
}

extern "C" int cheb_project_set_inverse_density(cheb_project *h, const double *kappa_dev, void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "project: NULL handle");
  if (!h->vh) return chebhip_fail(CHEBHIP_ERR_ARG, "project: set_inverse_density needs a handle of cheb_project_create_variable");
  return cheb_varhelm_set_coefficients(h->vh, kappa_dev, nullptr, 0.0, stream);
}

extern "C" int cheb_project_apply_variable(cheb_project *h, const double *u_dev, const double *flux_dev, double *phi_dev, double *out_dev, int warm,
                                           double rtol, double atol, int max_it, int restart, void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "project: NULL handle");
  if (!h->vh) return chebhip_fail(CHEBHIP_ERR_ARG, "project: apply_variable needs a handle of cheb_project_create_variable");
  if (cheb_varhelm_singular(h->vh) < 0) return chebhip_fail(CHEBHIP_ERR_ARG, "project: set_inverse_density has not been called");
  int rc;
  if ((rc = project_check(h, u_dev, flux_dev, phi_dev, out_dev))) return rc;
  const long N = h->N, G = h->G, NB = N - G;
  const double *kappa = varhelm_kappa(h->vh);
  hipStream_t st = (hipStream_t)stream;
  if ((rc = cheb_grad_div(h->grad, h->nvec, u_dev, phi_dev, stream))) return rc;
  hipLaunchKernelGGL(k_project_rhs<true>, dim3(grid1d(N, 256, 4096), (unsigned)h->nvec), dim3(256), 0, st, N, G, NB, h->d, h->open, h->map, h->face, phi_dev, u_dev,
                     flux_dev, kappa, h->f, h->g);
  sweep_note_launch();
  HIP_TRY(hipGetLastError());
  const bool guess = warm && h->have_x;
  h->have_x = false;
  if ((rc = cheb_varhelm_solve_deflated(h->vh, h->f, h->g, h->x, guess ? 1 : 0, phi_dev, rtol, atol, max_it, restart, stream))) return rc;
  h->have_x = true;
  if ((rc = cheb_grad_grad(h->grad, h->nvec, phi_dev, h->gw, stream))) return rc;
  if (NB) {
    hipLaunchKernelGGL(k_project_wall_grad, dim3(grid1d(N, 256, 4096), (unsigned)h->nvec), dim3(256), 0, st, N, NB, h->d, h->open, h->map, h->face,
                       (const double *)h->g, h->gw);
    sweep_note_launch();
  }
  const dim3 grid(grid1d(N / 2 > 0 ? N / 2 : 1, 256, 4096), (unsigned)(h->nvec * h->d));
  if ((N & 1) == 0 && ((((size_t)u_dev | (size_t)out_dev | (size_t)kappa | (size_t)h->gw) & 15) == 0))
    hipLaunchKernelGGL(k_project_correct<pj2>, grid, dim3(256), 0, st, N, kappa, (const double *)h->gw, u_dev, out_dev);
  else
    hipLaunchKernelGGL(k_project_correct<double>, dim3(grid1d(N, 256, 4096), grid.y), dim3(256), 0, st, N, kappa, (const double *)h->gw, u_dev, out_dev);
  sweep_note_launch();
  HIP_TRY(hipGetLastError());
  return 0;
}
