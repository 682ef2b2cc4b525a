// varhelm.hip -- the variable-coefficient Helmholtz operator  c(x) u - div( kappa(x) grad u )  on the conventions of the direct solve
// (cheb_varhelm_*, include/chebhip.h): the unknown layout, the faces, the scales, the periodic directions and the stacked
// fields of cheb_helmholtz_create_basis, with a preconditioned FGMRES solve behind one call.
//
// Operator.  For unknowns x and boundary data g
//   1. W = the full-grid extension of x: on every line of a wall direction k the two end values are Q_k x_line + B_BB^-1 g -- the very
//      launches the direct solve ends with (helmholtz_extend: bc_extend of precond.hip on this handle's arrays);
//   2. A = sum_k (-s_k^2) D_k( kappa . D_k W ) on the full grid, one direction after the other: one fused launch D(kappa . D W)
//      where the line's matrix fits the register-resident kernel (every CGL or Fourier line of at most 256 points), otherwise -- the
//      CGL lines of 257 and 258 points -- the gradient sweep (STORE) and the sweep with the flux multiply on its load side
//      (IN_FLUX_ETA); the first direction stores, the later ones accumulate (OUT_ACC);
//   3. y = c x + A at the unknown nodes (k_vh_close), or f - that for the residual.
// Lines of direction k whose other indices lie on a face run too (the sweeps take whole tensors): what they write lands on face
// nodes, which step 3 never reads, so edge and corner values of W influence nothing.  Every step is a line product or a pointwise
// pass over one field: a NaN in field j stays in field j, and nothing depends on timing -- the same call gives the same bits.
// kappa is kept as nfields stacked copies of the full grid (the flux multiply takes an array of its input's geometry); the
// preconditioner and the closing pass read copy 0 / the c field by index arithmetic from the unknown layout.
//
// Solve.  b = f - (operator at g)(0); FGMRES (krylov.hip) on A = the linear operator with the right preconditioner
// z = H(sigma_p)^-1 (r / kappa), H the direct solve of the same dims, basis, bc, scale and nfields, sigma_p = mean of c / kappa over
// the unknown nodes; the full-grid output by the same extension.
//
// Deflated solve.  With c == 0 and no Dirichlet or Robin face A is singular, its null space N known for any kappa (the
// constant and, per periodic direction of even extent, the Nyquist vector).  solve_deflated is the same FGMRES on Pi A with the
// preconditioner Pi H(0)^-1 (r / kappa), Pi = I - N N^T / G per field, between projections of b, of the guess and of the result;
// Pi is the three launches k_vh_null_partial, k_vh_null_total, k_vh_null_subtract below (fixed addition order, no atomics).
//
// Tensor mode (set_tensor).  c u + v . grad u - div( K grad u ), K a symmetric positive definite d x d tensor field
// (d = 2, 3), v a velocity field or none: the same extension, then G_k = s_k D_k W on the whole grid (d sweeps), the node pass
// k_vh_flux (F_j = sum_k K_jk G_k over G_j, a = sum_k v_k G_k into A), then A (+)= -s_j D_j F_j (d sweeps) and the same closing pass.
// Here the lines that lie on a face matter: F_j at a face node of direction j holds the tangential derivatives G_k of W on that
// face, whose end values are edge values of W -- those of the extension, every boundary node set once by the highest direction in
// which it is an end node.  The preconditioner and the solves are the scalar mode's on kappa = trace(K) / d.
#include "../../include/chebhip.h"
#include "ops.h"
#include "sweep.h"
#include <cmath>
#include <map>
#include <new>
#include <utility>
#include <vector>

using namespace chebhip;

namespace {

constexpr int VMAXD = 10;
typedef double vh2 __attribute__((ext_vector_type(2)));

// M[k] unknowns from full-grid index off[k] on (1 between walls, 0 on a periodic direction), row-major strides ls of the full grid;
// N, G per field.  32-bit: nfields N <= 2^31 - 1.
struct VhGeo { int d; int M[VMAXD]; int off[VMAXD]; int ls[VMAXD]; unsigned N, G; };

// the full-grid index of the first of the W consecutive unknowns q, q + 1, .. (W divides M[d-1]: they share a line of the last direction)
__device__ __forceinline__ unsigned vh_node(const VhGeo &g, unsigned q) {
  unsigned r = q, n = 0;
  for (int m = VMAXD - 1; m > 0; m--)
    if (m < g.d) { const unsigned Mm = (unsigned)g.M[m]; const unsigned i = r % Mm; r /= Mm; n += (i + (unsigned)g.off[m]) * (unsigned)g.ls[m]; }
  return n + (r + (unsigned)g.off[0]) * (unsigned)g.ls[0];
}
// W doubles from p: one 16-byte load where the address allows it, else two 8-byte ones
template <int W> struct VhVec;
template <> struct VhVec<1> {
  typedef double T;
  static __device__ __forceinline__ T load(const double *p) { return *p; }
  static __device__ __forceinline__ void store(double *p, T v) { *p = v; }
  static __device__ __forceinline__ T splat(double v) { return v; }
  static __device__ __forceinline__ double get(T v, int) { return v; }
  static __device__ __forceinline__ void sub(T &v, int, double c) { v -= c; }
};
template <> struct VhVec<2> {
  typedef vh2 T;
  static __device__ __forceinline__ T load(const double *p) {
    if (((size_t)p & 15) == 0) return *reinterpret_cast<const vh2 *>(p);
    return (vh2){p[0], p[1]};
  }
  static __device__ __forceinline__ void store(double *p, T v) { *reinterpret_cast<vh2 *>(p) = v; }      // unknown-layout side: aligned by the launcher
  static __device__ __forceinline__ T splat(double v) { return (vh2){v, v}; }
  static __device__ __forceinline__ double get(T v, int w) { return w ? v.y : v.x; }
  static __device__ __forceinline__ void sub(T &v, int w, double c) { if (w) v.y -= c; else v.x -= c; }
};

// The closing pass: out = c x + A at the unknown nodes (f null), or f - (c x + A) (the residual).  A: nfields full grids; cf: the c
// field on the full grid, or null and the scalar c0; field = blockIdx.y.  W = 2: M[d-1] even, x / f / out 16-byte aligned.
template <int W>
__global__ __launch_bounds__(256) void k_vh_close(VhGeo geo, const double *__restrict__ A, const double *__restrict__ cf, double c0,
                                                  const double *__restrict__ x, const double *__restrict__ f, double *__restrict__ out) {
  typedef VhVec<W> V;
  const unsigned per = geo.G / W;
  const size_t fu = (size_t)blockIdx.y * geo.G, fn = (size_t)blockIdx.y * geo.N;
  for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < per; t += gridDim.x * 256u) {
    const unsigned q = t * W, n = vh_node(geo, q);
    const typename V::T c = cf ? V::load(cf + n) : V::splat(c0);
    typename V::T v = c * V::load(x + fu + q) + V::load(A + fn + n);
    if (f) v = V::load(f + fu + q) - v;
    V::store(out + fu + q, v);
  }
}

// The first step of the preconditioner: t = r / kappa at the unknown nodes, kappa read from the full grid
template <int W>
__global__ __launch_bounds__(256) void k_vh_over_kappa(VhGeo geo, const double *__restrict__ r, const double *__restrict__ kappa, double *__restrict__ t) {
  typedef VhVec<W> V;
  const unsigned per = geo.G / W;
  const size_t fu = (size_t)blockIdx.y * geo.G;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < per; i += gridDim.x * 256u) {
    const unsigned q = i * W;
    V::store(t + fu + q, V::load(r + fu + q) / V::load(kappa + vh_node(geo, q)));
  }
}

// set_coefficients: part[b] = block b's share of sum c / kappa over the unknown nodes (fixed order: the host adds the VH_RB shares in
// turn), bad[b] = its count of full-grid nodes with kappa not finite or <= 0, or c not finite or < 0
constexpr int VH_RB = 256;
__global__ __launch_bounds__(256) void k_vh_coef_check(VhGeo geo, const double *__restrict__ kappa, const double *__restrict__ cf, double c0,
                                                       double *__restrict__ part, unsigned *__restrict__ bad) {
  __shared__ double sh[256];
  __shared__ unsigned shb[256];
  unsigned nb = 0;
  for (unsigned n = blockIdx.x * 256u + threadIdx.x; n < geo.N; n += gridDim.x * 256u) {
    const double k = kappa[n], c = cf ? cf[n] : c0;
    if (!(k > 0.0) || !(k - k == 0.0) || !(c >= 0.0) || !(c - c == 0.0)) nb++;
  }
  double s = 0.0;
  for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < geo.G; q += gridDim.x * 256u) {
    const unsigned n = vh_node(geo, q);
    s += (cf ? cf[n] : c0) / kappa[n];
  }
  sh[threadIdx.x] = s; shb[threadIdx.x] = nb;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { sh[threadIdx.x] += sh[threadIdx.x + o]; shb[threadIdx.x] += shb[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { part[blockIdx.x] = sh[0]; bad[blockIdx.x] = shb[0]; }
}

// ---- tensor mode -------------------------------------------------------------------------------------------------------
// K: d (d + 1) / 2 full grids, the diagonal first, then the upper triangle row-major (3-D: 00 11 22 01 02 12; 2-D: 00 11 01).
// The mean diagonal entry: what the preconditioner divides by
template <int D>
__device__ __forceinline__ double vh_kbar(const double *__restrict__ K, unsigned N, unsigned n) {
  double t = K[n] + K[(size_t)N + n];
  if (D == 3) t += K[2 * (size_t)N + n];
  return t / (double)D;
}
__device__ __forceinline__ bool vh_finite(double a) { return a - a == 0.0; }
// finite and positive definite by its leading principal minors
template <int D>
__device__ __forceinline__ bool vh_spd(const double *__restrict__ K, unsigned N, unsigned n) {
  const size_t s = N;
  if (D == 2) {
    const double k00 = K[n], k11 = K[s + n], k01 = K[2 * s + n];
    if (!vh_finite(k00) || !vh_finite(k11) || !vh_finite(k01)) return false;
    return k00 > 0.0 && k00 * k11 - k01 * k01 > 0.0;
  }
  const double k00 = K[n], k11 = K[s + n], k22 = K[2 * s + n], k01 = K[3 * s + n], k02 = K[4 * s + n], k12 = K[5 * s + n];
  if (!vh_finite(k00) || !vh_finite(k11) || !vh_finite(k22) || !vh_finite(k01) || !vh_finite(k02) || !vh_finite(k12)) return false;
  const double det = k00 * (k11 * k22 - k12 * k12) - k01 * (k01 * k22 - k12 * k02) + k02 * (k01 * k12 - k11 * k02);
  return k00 > 0.0 && k00 * k11 - k01 * k01 > 0.0 && det > 0.0;
}

// set_tensor: k_vh_coef_check for a tensor.  bad[b] = block b's count of full-grid nodes where K is not finite and positive
// definite, v (if given) or c not finite, or c < 0; kbar[n] = trace(K) / d at every node; part[b] = the block's share of
// sum c / kbar over the unknown nodes (a thread's nodes in turn, the block's tree, the host adds the VH_RB shares in turn)
template <int D>
__global__ __launch_bounds__(256) void k_vh_tensor_check(VhGeo geo, const double *__restrict__ K, const double *__restrict__ vel, const double *__restrict__ cf,
                                                         double c0, double *__restrict__ kbar, double *__restrict__ part, unsigned *__restrict__ bad) {
  __shared__ double sh[256];
  __shared__ unsigned shb[256];
  unsigned nb = 0;
  for (unsigned n = blockIdx.x * 256u + threadIdx.x; n < geo.N; n += gridDim.x * 256u) {
    bool ok = vh_spd<D>(K, geo.N, n);
    if (vel)
#pragma unroll
      for (int k = 0; k < D; k++) ok = ok && vh_finite(vel[(size_t)k * geo.N + n]);
    const double c = cf ? cf[n] : c0;
    if (!ok || !(c >= 0.0) || !vh_finite(c)) nb++;
    kbar[n] = vh_kbar<D>(K, geo.N, n);
  }
  double s = 0.0;
  for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < geo.G; q += gridDim.x * 256u) {
    const unsigned n = vh_node(geo, q);
    s += (cf ? cf[n] : c0) / vh_kbar<D>(K, geo.N, n);
  }
  sh[threadIdx.x] = s; shb[threadIdx.x] = nb;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { sh[threadIdx.x] += sh[threadIdx.x + o]; shb[threadIdx.x] += shb[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { part[blockIdx.x] = sh[0]; bad[blockIdx.x] = shb[0]; }
}

// two consecutive doubles (two = false: the first alone, the last node of an odd grid): one 16-byte access where the address
// allows it -- the stacked grids of an odd N put every other field on an 8-byte boundary -- else 8-byte ones
__device__ __forceinline__ vh2 vh_ld2(const double *p, bool two) {
  if (two && ((size_t)p & 15) == 0) return *reinterpret_cast<const vh2 *>(p);
  return (vh2){p[0], two ? p[1] : 0.0};
}
__device__ __forceinline__ void vh_st2(double *p, vh2 v, bool two) {
  if (two && ((size_t)p & 15) == 0) { *reinterpret_cast<vh2 *>(p) = v; return; }
  p[0] = v.x;
  if (two) p[1] = v.y;
}
// sum_k a_k g_k, k ascending: one product, then fused multiply-adds, written out -- D roundings whatever the compiler's
// contraction setting and whatever the width of the accesses around it
__device__ __forceinline__ double vh_dot2(double a0, double a1, double g0, double g1) { return __builtin_fma(a1, g1, a0 * g0); }
__device__ __forceinline__ double vh_dot3(double a0, double a1, double a2, double g0, double g1, double g2) {
  return __builtin_fma(a2, g2, __builtin_fma(a1, g1, a0 * g0));
}

// The node pass of the tensor mode, field = blockIdx.y, a lane per pair of neighbouring nodes of the full grid: G_k = Gt + k gs
// (k < D) are the scaled gradients of the nf stacked fields; on return G_j holds F_j = sum_k K_jk G_k and, with a velocity, A
// holds a = sum_k v_k G_k.  K and vel are indexed by node (one copy for all fields).  A lane reads all it needs before its first
// store and no lane reads another's nodes: in place.  No LDS, no atomics; the sums are vh_dot2 / vh_dot3 (explicit fused
// multiply-adds), so their rounding does not depend on the access width.
template <int D, bool VEL>
__global__ __launch_bounds__(256) void k_vh_flux(unsigned N, size_t gs, const double *__restrict__ K, const double *__restrict__ vel,
                                                 double *Gt, double *__restrict__ A) {
  const unsigned per = (N + 1u) / 2u;
  const size_t fo = (size_t)blockIdx.y * N, s = N;
  for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < per; t += gridDim.x * 256u) {
    const unsigned n = 2u * t;
    const bool two = n + 1u < N;
    double *g = Gt + fo + n;
    const vh2 g0 = vh_ld2(g, two), g1 = vh_ld2(g + gs, two);
    const vh2 k00 = vh_ld2(K + n, two), k11 = vh_ld2(K + s + n, two);
    if (D == 2) {
      const vh2 k01 = vh_ld2(K + 2 * s + n, two);
      vh2 a = {0.0, 0.0};
      if (VEL) {
        const vh2 v0 = vh_ld2(vel + n, two), v1 = vh_ld2(vel + s + n, two);
        a = (vh2){vh_dot2(v0.x, v1.x, g0.x, g1.x), vh_dot2(v0.y, v1.y, g0.y, g1.y)};
      }
      const vh2 f0 = {vh_dot2(k00.x, k01.x, g0.x, g1.x), vh_dot2(k00.y, k01.y, g0.y, g1.y)};
      const vh2 f1 = {vh_dot2(k01.x, k11.x, g0.x, g1.x), vh_dot2(k01.y, k11.y, g0.y, g1.y)};
      vh_st2(g, f0, two); vh_st2(g + gs, f1, two);
      if (VEL) vh_st2(A + fo + n, a, two);
    } else {
      const vh2 g2 = vh_ld2(g + 2 * gs, two);
      const vh2 k22 = vh_ld2(K + 2 * s + n, two), k01 = vh_ld2(K + 3 * s + n, two), k02 = vh_ld2(K + 4 * s + n, two), k12 = vh_ld2(K + 5 * s + n, two);
      vh2 a = {0.0, 0.0};
      if (VEL) {
        const vh2 v0 = vh_ld2(vel + n, two), v1 = vh_ld2(vel + s + n, two), v2 = vh_ld2(vel + 2 * s + n, two);
        a = (vh2){vh_dot3(v0.x, v1.x, v2.x, g0.x, g1.x, g2.x), vh_dot3(v0.y, v1.y, v2.y, g0.y, g1.y, g2.y)};
      }
      const vh2 f0 = {vh_dot3(k00.x, k01.x, k02.x, g0.x, g1.x, g2.x), vh_dot3(k00.y, k01.y, k02.y, g0.y, g1.y, g2.y)};
      const vh2 f1 = {vh_dot3(k01.x, k11.x, k12.x, g0.x, g1.x, g2.x), vh_dot3(k01.y, k11.y, k12.y, g0.y, g1.y, g2.y)};
      const vh2 f2 = {vh_dot3(k02.x, k12.x, k22.x, g0.x, g1.x, g2.x), vh_dot3(k02.y, k12.y, k22.y, g0.y, g1.y, g2.y)};
      vh_st2(g, f0, two); vh_st2(g + gs, f1, two); vh_st2(g + 2 * gs, f2, two);
      if (VEL) vh_st2(A + fo + n, a, two);
    }
  }
}

// ---- the projection Pi = I - N N^T / G of the deflated solve ------------------------------------------------------------
// The null space of a singular handle: the m even periodic directions dir[0] < dir[1] < .. (m <= 3); null vector j of the q = 2^m
// alternates, (-1)^index, in dir[b] for every bit b of j.  Vector 0 is the constant.
struct VhNull { int m; int dir[3]; };
constexpr int VH_PB = 512;                     // blocks of the partial pass per field
constexpr int VH_TS = 24;                      // doubles per field of a totals array: [0, 8) the sums, [8, 16) the sums / G, [16] 1 = subtract
constexpr double VH_U = 1.1102230246251565e-16;

// bit b: the parity of unknown q's index in direction dir[b]
__device__ __forceinline__ unsigned vh_parity(const VhGeo &g, const VhNull &z, unsigned q) {
  unsigned r = q, p = 0;
  int b = z.m - 1;
  for (int m = VMAXD - 1; m > 0; m--)
    if (m < g.d) {
      const unsigned Mm = (unsigned)g.M[m]; const unsigned i = r % Mm; r /= Mm;
      if (b >= 0 && z.dir[b] == m) { p |= (i & 1u) << b; b--; }
    }
  if (b >= 0) p |= (r & 1u) << b;              // (dir[0] == 0)
  return p;
}
__device__ __forceinline__ double vh_signed(unsigned j, unsigned p, double v) { return (__popc(j & p) & 1) ? -v : v; }

// the sums of a block of 256 in a fixed order: sh[j][0] = the tree 128, 64, .. 1 over the threads' values
template <int R>
__device__ __forceinline__ void vh_block_tree(double (&sh)[R][256]) {
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
#pragma unroll
      for (int j = 0; j < R; j++) sh[j][threadIdx.x] += sh[j][threadIdx.x + o];
    __syncthreads();
  }
}

// First pass: part[(field (Q + 1) + j) VH_PB + block] = the block's share of z_j^T x (j < Q) and of sum |x| (j = Q); a thread adds
// its elements in ascending order.  W = 2: pairs along the last direction (M[d-1] even, so the first of a pair has an even index).
template <int W, int Q>
__global__ __launch_bounds__(256) void k_vh_null_partial(VhGeo geo, VhNull z, const double *__restrict__ in, double *__restrict__ part) {
  typedef VhVec<W> V;
  __shared__ double sh[Q + 1][256];
  const unsigned per = geo.G / W;
  const size_t fu = (size_t)blockIdx.y * geo.G;
  const unsigned pairbit = (Q > 1 && W == 2 && z.dir[z.m - 1] == geo.d - 1) ? 1u << (z.m - 1) : 0u;
  double s[Q + 1];
#pragma unroll
  for (int j = 0; j <= Q; j++) s[j] = 0.0;
  for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < per; t += (unsigned)VH_PB * 256u) {
    const unsigned q = t * W, p = Q > 1 ? vh_parity(geo, z, q) : 0u;
    const typename V::T v = V::load(in + fu + q);
#pragma unroll
    for (int w = 0; w < W; w++) {
      const double x = V::get(v, w);
      const unsigned pw = w ? p ^ pairbit : p;
#pragma unroll
      for (int j = 0; j < Q; j++) s[j] += vh_signed((unsigned)j, pw, x);
      s[Q] += fabs(x);
    }
  }
#pragma unroll
  for (int j = 0; j <= Q; j++) sh[j][threadIdx.x] = s[j];
  vh_block_tree(sh);
  if (threadIdx.x == 0)
#pragma unroll
    for (int j = 0; j <= Q; j++) part[((size_t)blockIdx.y * (Q + 1) + j) * VH_PB + blockIdx.x] = sh[j][0];
}

// Second pass, one block per field: the VH_PB shares in a fixed order (share t + share t + 256, then the tree), the coefficients
// s_j / G, and whether the third pass subtracts: not where every |s_j| <= tau sum |x| -- x is in the range of Pi already as far as
// Pi can bring it there, and stays bit for bit
template <int Q>
__global__ __launch_bounds__(256) void k_vh_null_total(const double *__restrict__ part, double G, double tau, double *__restrict__ tot) {
  __shared__ double sh[Q + 1][256];
  const double *pf = part + (size_t)blockIdx.x * (Q + 1) * VH_PB;
#pragma unroll
  for (int j = 0; j <= Q; j++) sh[j][threadIdx.x] = pf[j * VH_PB + threadIdx.x] + pf[j * VH_PB + threadIdx.x + 256];
  vh_block_tree(sh);
  if (threadIdx.x == 0) {
    double *tf = tot + (size_t)blockIdx.x * VH_TS;
    bool keep = true;
    for (int j = 0; j < Q; j++) {
      tf[j] = sh[j][0]; tf[8 + j] = sh[j][0] / G;
      keep = keep && fabs(sh[j][0]) <= tau * sh[Q][0];
    }
    tf[16] = keep ? 0.0 : 1.0;
  }
}

// Third pass: out = in - sum_j z_j (s_j / G), the correction added up over j ascending and subtracted once; in == out allowed
template <int W, int Q>
__global__ __launch_bounds__(256) void k_vh_null_subtract(VhGeo geo, VhNull z, const double *__restrict__ tot, const double *in, double *out) {
  typedef VhVec<W> V;
  const unsigned per = geo.G / W;
  const size_t fu = (size_t)blockIdx.y * geo.G;
  const double *tf = tot + (size_t)blockIdx.y * VH_TS;
  const bool sub = tf[16] != 0.0;
  if (!sub && in == out) return;
  const unsigned pairbit = (Q > 1 && W == 2 && z.dir[z.m - 1] == geo.d - 1) ? 1u << (z.m - 1) : 0u;
  double c[Q];
#pragma unroll
  for (int j = 0; j < Q; j++) c[j] = tf[8 + j];
  for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < per; t += gridDim.x * 256u) {
    const unsigned q = t * W;
    typename V::T v = V::load(in + fu + q);
    if (sub) {
      const unsigned p = Q > 1 ? vh_parity(geo, z, q) : 0u;
#pragma unroll
      for (int w = 0; w < W; w++) {
        const unsigned pw = w ? p ^ pairbit : p;
        double corr = c[0];
#pragma unroll
        for (int j = 1; j < Q; j++) corr += vh_signed((unsigned)j, pw, c[j]);
        V::sub(v, w, corr);
      }
    }
    V::store(out + fu + q, v);
  }
}

}  // namespace

struct cheb_varhelm {
  int d = 0, nf = 1;
  int P[VMAXD] = {0}, basis[VMAXD] = {0};
  double s2[VMAXD] = {0};                      // fl(s_k s_k): the factor of direction k is alpha = -s2[k]
  double s1[VMAXD] = {0};                      // s_k: the factor of both sweeps of the tensor mode
  unsigned inner[VMAXD] = {0};
  VhGeo geo = {};
  long N = 0, G = 0, NB = 0;
  cheb_helmholtz *H = nullptr;                 // the preconditioner's direct solve; also the lines of the extension
  std::map<std::pair<int, int>, DiffMat> D;    // by (extent, basis)
  const DiffMat *Dk[VMAXD] = {nullptr};
  double *Wf = nullptr, *Gk = nullptr, *A = nullptr;   // nf full grids each: the extension, one gradient, the sum
  double *kap = nullptr;                       // nf stacked copies of kappa
  double *cfield = nullptr; double c0 = 0.0; bool c_is_field = false;
  int mode = 0;                                // CHEB_VARHELM_MODE_*: none, scalar (set_coefficients), tensor (set_tensor)
  double *Kt = nullptr, *vel = nullptr;        // tensor mode, made by the first set_tensor: d (d + 1) / 2 and d full grids, one copy for all fields
  double *Gt = nullptr;                        // ... and d gradient grids of nf fields each
  bool has_vel = false;
  double *tu = nullptr, *bu = nullptr, *zero = nullptr;  // nf G each: r / kappa, the solve's right-hand side, a zero vector
  double *part = nullptr; unsigned *bad = nullptr;
  VhNull null = {};                            // the even periodic directions; null.m > 3: the deflated calls refuse
  double *npart = nullptr, *ntot = nullptr, *dtot = nullptr;   // the projection's block shares and totals; the totals of the last defect
  int defect_q = 0;                            // null vectors of the last deflated solve (0: none yet, or a nonsingular one)
  bool have_coef = false, any_two_sweeps = false;
  double sigma_p = 0.0;
  chebhip_fgmres *krylov = nullptr; int krylov_restart = 0;   // made by the first solve; a solve with another restart length replaces it
  int iterations = 0, reason = 0; double residual = 0.0;
  size_t own_bytes = 0, krylov_bytes = 0;
};

namespace {

// the fused launch takes every matrix the register-resident kernels hold: diffmat.cpp gives KS <= 32 to every line of at most 256
// points (H = ceil(P / 2) <= 128); KS = 0 is a long line (257, 258 points here)
bool vh_fused(const DiffMat &m) { return m.KS == 4 || m.KS == 8 || m.KS == 16 || m.KS == 32; }

int vh_alloc(cheb_varhelm *h, double **p, size_t n) {
  const size_t bytes = (n ? n : 1) * sizeof(double);
  if (hipMalloc((void **)p, bytes) != hipSuccess) { *p = nullptr; (void)hipGetLastError(); return chebhip_fail(CHEBHIP_ERR_MEMORY, "out of device memory (%zu bytes)", bytes); }
  h->own_bytes += bytes;
  return 0;
}

template <class K, class... Args>
void vh_launch_rows(K kern1, K kern2, bool vec, const cheb_varhelm *h, hipStream_t st, Args... args) {
  const unsigned per = h->geo.G / (vec ? 2u : 1u);
  const dim3 grid(grid1d(per, 256, 4096), (unsigned)h->nf);
  hipLaunchKernelGGL(vec ? kern2 : kern1, grid, dim3(256), 0, st, h->geo, args...);
  sweep_note_launch();
}
bool vh_pairs(const cheb_varhelm *h, const double *a, const double *b, const double *c) {
  return (h->geo.M[h->d - 1] & 1) == 0 && ((((size_t)a | (size_t)b | (size_t)c) & 15) == 0);
}

// A = sum_k -s_k^2 D_k( kappa D_k W ) on nf full grids
int vh_flux_sum(cheb_varhelm *h, const double *W, hipStream_t st) {
  for (int k = 0; k < h->d; k++) {
    const DiffMat &m = *h->Dk[k];
    SweepParams sp = {};
    sp.ncols = (unsigned)((long)h->nf * h->N / h->P[k]); sp.inner = h->inner[k];
    sp.alpha = -h->s2[k]; sp.out = h->A;
    if (k > 0) { sp.out_mode = OUT_ACC; sp.acc = h->A; } else sp.out_mode = OUT_STORE;
    if (vh_fused(m)) {
      sp.in0 = W; sp.in_mode = IN_PLAIN; sp.coef_mode = COEF_ETA; sp.in1 = h->kap;
      HIP_TRY(fused_launch(m, sp, st));
      continue;
    }
    SweepParams sg = {};
    sg.ncols = sp.ncols; sg.inner = sp.inner; sg.in0 = W; sg.in_mode = IN_PLAIN; sg.alpha = 1.0; sg.out = h->Gk; sg.out_mode = OUT_STORE;
    HIP_TRY(sweep_launch(m, sg, st));
    sp.in0 = h->Gk; sp.in1 = h->kap; sp.in_mode = IN_FLUX_ETA;
    HIP_TRY(sweep_launch(m, sp, st));
  }
  return 0;
}

// tensor mode: A = sum_k v_k G_k - sum_j s_j D_j( sum_k K_jk G_k ), G_k = s_k D_k W, on nf full grids
int vh_tensor_sum(cheb_varhelm *h, const double *W, hipStream_t st) {
  const size_t gs = (size_t)h->nf * h->N;
  SweepParams sp = {};
  for (int k = 0; k < h->d; k++) {
    sp.ncols = (unsigned)((long)h->nf * h->N / h->P[k]); sp.inner = h->inner[k];
    sp.in0 = W; sp.in_mode = IN_PLAIN; sp.alpha = h->s1[k]; sp.out = h->Gt + k * gs; sp.out_mode = OUT_STORE; sp.acc = nullptr;
    HIP_TRY(sweep_launch(*h->Dk[k], sp, st));
  }
  const dim3 grid(grid1d(((long)h->N + 1) / 2, 256, 4096), (unsigned)h->nf);
  const unsigned N = (unsigned)h->N;
  if (h->d == 2) {
    if (h->has_vel) hipLaunchKernelGGL((k_vh_flux<2, true>), grid, dim3(256), 0, st, N, gs, (const double *)h->Kt, (const double *)h->vel, h->Gt, h->A);
    else hipLaunchKernelGGL((k_vh_flux<2, false>), grid, dim3(256), 0, st, N, gs, (const double *)h->Kt, (const double *)nullptr, h->Gt, h->A);
  } else {
    if (h->has_vel) hipLaunchKernelGGL((k_vh_flux<3, true>), grid, dim3(256), 0, st, N, gs, (const double *)h->Kt, (const double *)h->vel, h->Gt, h->A);
    else hipLaunchKernelGGL((k_vh_flux<3, false>), grid, dim3(256), 0, st, N, gs, (const double *)h->Kt, (const double *)nullptr, h->Gt, h->A);
  }
  sweep_note_launch();
  HIP_TRY(hipGetLastError());
  for (int j = 0; j < h->d; j++) {
    sp.ncols = (unsigned)((long)h->nf * h->N / h->P[j]); sp.inner = h->inner[j];
    sp.in0 = h->Gt + j * gs; sp.alpha = -h->s1[j]; sp.out = h->A;
    if (j > 0 || h->has_vel) { sp.out_mode = OUT_ACC; sp.acc = h->A; } else { sp.out_mode = OUT_STORE; sp.acc = nullptr; }
    HIP_TRY(sweep_launch(*h->Dk[j], sp, st));
  }
  return 0;
}

// out = (operator at g)(x), or f - that
int vh_operator(cheb_varhelm *h, const double *x, const double *f, const double *g, double *out, hipStream_t st) {
  if (!h->have_coef) return chebhip_fail(CHEBHIP_ERR_ARG, "cheb_varhelm: set_coefficients has not been called");
  const double *W = x;                         // no wall: the unknown layout is the full grid
  if (h->NB) { int rc = helmholtz_extend(h->H, x, g, h->Wf, st); if (rc) return rc; W = h->Wf; }
  int rc = h->mode == CHEB_VARHELM_MODE_TENSOR ? vh_tensor_sum(h, W, st) : vh_flux_sum(h, W, st); if (rc) return rc;
  const bool vec = vh_pairs(h, x, f, out);
  vh_launch_rows(k_vh_close<1>, k_vh_close<2>, vec, h, st, (const double *)h->A, (const double *)(h->c_is_field ? h->cfield : nullptr), h->c0, x, f, out);
  HIP_TRY(hipGetLastError());
  return 0;
}

int vh_check_vectors(const cheb_varhelm *h, const char *what, const double *x, const double *f, const double *g, const double *out) {
  const long n = (long)h->nf * h->G, nb = (long)h->nf * h->NB;
  if (!x || !out) return chebhip_fail(CHEBHIP_ERR_ARG, "%s: NULL vector", what);
  if (g && h->NB == 0) return chebhip_fail(CHEBHIP_ERR_ARG, "%s: g given, but every direction is periodic: there is no boundary data", what);
  if (overlap(out, n, x, n) || (f && overlap(out, n, f, n)) || (g && overlap(out, n, g, nb)))
    return chebhip_fail(CHEBHIP_ERR_ARG, "%s: out may not alias x, f or g", what);
  return 0;
}

// the even periodic directions of a geometry, ascending; returns their number (any number: the callers check the limit of 3)
int vh_even_periodic(int d, const int *dims, const int *basis, int *dir3) {
  int m = 0;
  for (int k = 0; k < d; k++)
    if (basis && basis[k] == BASIS_FOURIER && (dims[k] & 1) == 0) { if (m < 3) dir3[m] = k; m++; }
  return m;
}

// q of the handle as its coefficients stand: 0 nonsingular, 2^m singular; -1 with the error set: more than three even periodic directions
int vh_null_count(const cheb_varhelm *h, const char *what) {
  if (!cheb_helmholtz_singular(h->H)) return 0;
  if (h->null.m > 3) {
    chebhip_fail(CHEBHIP_ERR_ARG, "%s: %d even periodic directions give %ld null vectors: more than three such directions (8 vectors) are not supported", what, h->null.m, 1L << h->null.m);
    return -1;
  }
  return 1 << h->null.m;
}

// (Depth of the fixed addition order of one of these sums, the T of DESIGN 10q: a thread's elements in turn, at most
// 2 ceil(G / (2 VH_PB 256)); the block's tree, 8; the pair of shares, 1; the tree over them, 8.)
template <int Q>
void vh_null_launch(const cheb_varhelm *h, bool vec, const double *in, double *out, double *tot, double tau, hipStream_t st) {
  const dim3 pgrid(VH_PB, (unsigned)h->nf);
  if (vec) hipLaunchKernelGGL((k_vh_null_partial<2, Q>), pgrid, dim3(256), 0, st, h->geo, h->null, in, h->npart);
  else hipLaunchKernelGGL((k_vh_null_partial<1, Q>), pgrid, dim3(256), 0, st, h->geo, h->null, in, h->npart);
  sweep_note_launch();
  hipLaunchKernelGGL((k_vh_null_total<Q>), dim3((unsigned)h->nf), dim3(256), 0, st, (const double *)h->npart, (double)h->G, tau, tot);
  sweep_note_launch();
  if (out) vh_launch_rows(k_vh_null_subtract<1, Q>, k_vh_null_subtract<2, Q>, vec, h, st, h->null, (const double *)tot, in, out);
}

// out = Pi in (in == out allowed), or with out null the sums alone, into the totals array tot; q = 1, 2, 4 or 8
int vh_remove_null(cheb_varhelm *h, int q, const double *in, double *out, double *tot, hipStream_t st) {
  if (h->G == 0) return 0;
  const bool vec = vh_pairs(h, in, out, nullptr);
  // every computed |s_j| <= (q + 4) U sum |x|: with the sums' own error T U sum |x| the true ones are within the (T + q + 4) U sum |x|
  // that a subtraction guarantees, and x is left as it is
  const double tau = (double)(q + 4) * VH_U;
  switch (q) {
    case 1: vh_null_launch<1>(h, vec, in, out, tot, tau, st); break;
    case 2: vh_null_launch<2>(h, vec, in, out, tot, tau, st); break;
    case 4: vh_null_launch<4>(h, vec, in, out, tot, tau, st); break;
    default: vh_null_launch<8>(h, vec, in, out, tot, tau, st); break;
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int cheb_varhelm_destroy(cheb_varhelm *h) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (h->krylov) chebhip_fgmres_destroy(h->krylov);
  if (h->H) cheb_helmholtz_destroy(h->H);
  for (auto &kv : h->D) diffmat_destroy(&kv.second);
  double *all[] = {h->Wf, h->Gk, h->A, h->kap, h->cfield, h->tu, h->bu, h->zero, h->part, h->npart, h->ntot, h->dtot, h->Kt, h->vel, h->Gt};
  for (double *p : all) if (p) (void)hipFree(p);
  if (h->bad) (void)hipFree(h->bad);
  delete h;
  return 0;
}

extern "C" int cheb_varhelm_create(int d, const int *dims, const int *basis, const double *bc, const double *scale, int nfields, cheb_varhelm **out) {
  if (!out) return chebhip_fail(CHEBHIP_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (!dims || d < 1 || d > VMAXD) return chebhip_fail(CHEBHIP_ERR_DIMS, "d = %d must be in 1..10", d);
  // the argument checks, limits and lines are the direct solve's: its handle is made first (sigma 0 until set_coefficients)
  cheb_helmholtz *H = nullptr;
  std::vector<int> cgl(d, BASIS_CGL);
  int rc = cheb_helmholtz_create_basis(d, dims, basis ? basis : cgl.data(), bc, scale, 0.0, nfields, &H);
  if (rc) return rc;
  cheb_varhelm *h = new (std::nothrow) cheb_varhelm;
  if (!h) { cheb_helmholtz_destroy(H); return chebhip_fail(CHEBHIP_ERR_MEMORY, "out of host memory"); }
  h->H = H; h->d = d; h->nf = nfields;
  VhGeo &geo = h->geo;
  geo.d = d;
  long N = 1, G = 1;
  for (int k = d - 1; k >= 0; k--) {
    h->P[k] = dims[k]; h->basis[k] = basis ? basis[k] : BASIS_CGL;
    const double s = scale ? scale[k] : 1.0;
    h->s2[k] = s * s; h->s1[k] = s;
    h->inner[k] = (unsigned)N;
    geo.off[k] = h->basis[k] == BASIS_FOURIER ? 0 : 1; geo.M[k] = dims[k] - 2 * geo.off[k]; geo.ls[k] = (int)N;
    N *= dims[k]; G *= geo.M[k];
  }
  h->N = N; h->G = G; h->NB = N - G; geo.N = (unsigned)N; geo.G = (unsigned)G;
  for (int k = 0; k < d; k++) {
    const std::pair<int, int> key(dims[k], h->basis[k]);
    if (!h->D.count(key)) {
      DiffMat m;
      HIP_TRY_OR(h->basis[k] == BASIS_FOURIER ? diffmat_create_fourier(dims[k], 1, &m) : diffmat_create(dims[k], &m), cheb_varhelm_destroy(h));
      h->D[key] = m;
    }
    h->Dk[k] = &h->D.at(key);
    h->any_two_sweeps = h->any_two_sweeps || !vh_fused(*h->Dk[k]);
  }
  const size_t nN = (size_t)nfields * N, nG = (size_t)nfields * G;
  if ((h->NB && (rc = vh_alloc(h, &h->Wf, nN))) || (h->any_two_sweeps && (rc = vh_alloc(h, &h->Gk, nN))) || (rc = vh_alloc(h, &h->A, nN)) ||
      (rc = vh_alloc(h, &h->kap, nN)) || (rc = vh_alloc(h, &h->cfield, (size_t)N)) || (rc = vh_alloc(h, &h->tu, nG)) || (rc = vh_alloc(h, &h->bu, nG)) ||
      (rc = vh_alloc(h, &h->zero, nG)) || (rc = vh_alloc(h, &h->part, VH_RB))) { cheb_varhelm_destroy(h); return rc; }
  // the projection of the deflated solve, where the geometry can be singular at all (no Dirichlet or Robin face: cheb_helmholtz_singular
  // at sigma = 0) and has at most 8 null vectors
  h->null.m = vh_even_periodic(d, dims, basis, h->null.dir);
  if (cheb_helmholtz_singular(H) && h->null.m <= 3) {
    const size_t q1 = (size_t)(1 << h->null.m) + 1;
    if ((rc = vh_alloc(h, &h->npart, (size_t)nfields * q1 * VH_PB)) || (rc = vh_alloc(h, &h->ntot, (size_t)nfields * VH_TS)) ||
        (rc = vh_alloc(h, &h->dtot, (size_t)nfields * VH_TS))) { cheb_varhelm_destroy(h); return rc; }
  }
  HIP_TRY_OR(hipMalloc((void **)&h->bad, VH_RB * sizeof(unsigned)), cheb_varhelm_destroy(h));
  HIP_TRY_OR(hipMemset(h->zero, 0, (nG ? nG : 1) * sizeof(double)), cheb_varhelm_destroy(h));
  *out = h;
  return 0;
}

extern "C" long cheb_varhelm_size(const cheb_varhelm *h) { return h ? (long)h->nf * h->G : -1; }
extern "C" long cheb_varhelm_full_size(const cheb_varhelm *h) { return h ? (long)h->nf * h->N : -1; }
extern "C" long cheb_varhelm_boundary_size(const cheb_varhelm *h) { return h ? (long)h->nf * h->NB : -1; }
extern "C" long cheb_varhelm_work_bytes(const cheb_varhelm *h) { return h ? (long)(h->own_bytes + h->krylov_bytes + helmholtz_work_bytes(h->H)) : -1; }
const double *varhelm_kappa(const cheb_varhelm *h) { return h->kap; }
extern "C" int cheb_varhelm_singular(const cheb_varhelm *h) { return h && h->have_coef ? cheb_helmholtz_singular(h->H) : -1; }
extern "C" double cheb_varhelm_sigma(const cheb_varhelm *h) { return h && h->have_coef ? h->sigma_p : -1.0; }

extern "C" int cheb_varhelm_set_coefficients(cheb_varhelm *h, const double *kappa_dev, const double *c_dev, double c_scalar, void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (!kappa_dev) return chebhip_fail(CHEBHIP_ERR_ARG, "kappa is NULL");
  if (!c_dev && (!(c_scalar >= 0.0) || !std::isfinite(c_scalar))) return chebhip_fail(CHEBHIP_ERR_ARG, "c = %g must be finite and >= 0", c_scalar);
  hipStream_t st = (hipStream_t)stream;
  // checked on the caller's arrays before anything of the handle changes: a refused call leaves the earlier coefficients in place
  hipLaunchKernelGGL(k_vh_coef_check, dim3(VH_RB), dim3(256), 0, st, h->geo, kappa_dev, c_dev, c_scalar, h->part, h->bad);
  HIP_TRY(hipGetLastError());
  double part[VH_RB]; unsigned bad[VH_RB];
  HIP_TRY(hipMemcpyAsync(part, h->part, sizeof(part), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(bad, h->bad, sizeof(bad), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipDeviceSynchronize());               // also: no earlier solve of this handle is still reading what changes below
  double s = 0.0; unsigned long nbad = 0;
  for (int b = 0; b < VH_RB; b++) { s += part[b]; nbad += bad[b]; }
  if (nbad) return chebhip_fail(CHEBHIP_ERR_ARG, "set_coefficients: %lu nodes where kappa is not finite and > 0 or c is not finite and >= 0", nbad);
  const double sigma = h->G ? s / (double)h->G : 0.0;
  int rc = helmholtz_set_sigma(h->H, sigma); if (rc) return rc;
  for (int f = 0; f < h->nf; f++)
    HIP_TRY(hipMemcpyAsync(h->kap + (size_t)f * h->N, kappa_dev, (size_t)h->N * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (c_dev) HIP_TRY(hipMemcpyAsync(h->cfield, c_dev, (size_t)h->N * sizeof(double), hipMemcpyDeviceToDevice, st));
  h->c_is_field = c_dev != nullptr; h->c0 = c_dev ? 0.0 : c_scalar;
  HIP_TRY(hipStreamSynchronize(st));              // the call is synchronous: the copies are complete for every stream when it returns
  h->sigma_p = sigma; h->have_coef = true; h->mode = CHEB_VARHELM_MODE_SCALAR;
  return 0;
}

extern "C" int cheb_varhelm_mode(const cheb_varhelm *h) { return h ? h->mode : -1; }

extern "C" int cheb_varhelm_set_tensor(cheb_varhelm *h, const double *K_dev, const double *vel_dev, const double *c_dev, double c_scalar, void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (h->d != 2 && h->d != 3) return chebhip_fail(CHEBHIP_ERR_ARG, "set_tensor: d = %d; the tensor mode exists for d = 2 and d = 3", h->d);
  if (!K_dev) return chebhip_fail(CHEBHIP_ERR_ARG, "K is NULL");
  if (!c_dev && (!(c_scalar >= 0.0) || !std::isfinite(c_scalar))) return chebhip_fail(CHEBHIP_ERR_ARG, "c = %g must be finite and >= 0", c_scalar);
  hipStream_t st = (hipStream_t)stream;
  const int d = h->d, nk = d * (d + 1) / 2;
  const size_t N = (size_t)h->N;
  int rc;
  if ((!h->Kt && (rc = vh_alloc(h, &h->Kt, nk * N))) || (!h->vel && (rc = vh_alloc(h, &h->vel, d * N))) ||
      (!h->Gt && (rc = vh_alloc(h, &h->Gt, d * (size_t)h->nf * N)))) return rc;
  // no earlier call of this handle is still using the gradient grids: the check leaves trace(K) / d in the first of them, and
  // nothing of the handle's coefficients changes before it has passed
  HIP_TRY(hipDeviceSynchronize());
  if (d == 2) hipLaunchKernelGGL(k_vh_tensor_check<2>, dim3(VH_RB), dim3(256), 0, st, h->geo, K_dev, vel_dev, c_dev, c_scalar, h->Gt, h->part, h->bad);
  else hipLaunchKernelGGL(k_vh_tensor_check<3>, dim3(VH_RB), dim3(256), 0, st, h->geo, K_dev, vel_dev, c_dev, c_scalar, h->Gt, h->part, h->bad);
  HIP_TRY(hipGetLastError());
  double part[VH_RB]; unsigned bad[VH_RB];
  HIP_TRY(hipMemcpyAsync(part, h->part, sizeof(part), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(bad, h->bad, sizeof(bad), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipDeviceSynchronize());
  double s = 0.0; unsigned long nbad = 0;
  for (int b = 0; b < VH_RB; b++) { s += part[b]; nbad += bad[b]; }
  if (nbad) return chebhip_fail(CHEBHIP_ERR_ARG, "set_tensor: %lu nodes where K is not finite and positive definite, v is not finite or c is not finite and >= 0", nbad);
  const double sigma = h->G ? s / (double)h->G : 0.0;
  rc = helmholtz_set_sigma(h->H, sigma); if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(h->kap, h->Gt, N * sizeof(double), hipMemcpyDeviceToDevice, st));     // copy 0: all the preconditioner reads
  HIP_TRY(hipMemcpyAsync(h->Kt, K_dev, nk * N * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (vel_dev) HIP_TRY(hipMemcpyAsync(h->vel, vel_dev, d * N * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (c_dev) HIP_TRY(hipMemcpyAsync(h->cfield, c_dev, N * sizeof(double), hipMemcpyDeviceToDevice, st));
  h->c_is_field = c_dev != nullptr; h->c0 = c_dev ? 0.0 : c_scalar; h->has_vel = vel_dev != nullptr;
  HIP_TRY(hipStreamSynchronize(st));
  h->sigma_p = sigma; h->have_coef = true; h->mode = CHEB_VARHELM_MODE_TENSOR;
  return 0;
}

extern "C" int cheb_varhelm_mult(cheb_varhelm *h, const double *x_dev, double *y_dev, void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  int rc = vh_check_vectors(h, "mult", x_dev, nullptr, nullptr, y_dev); if (rc) return rc;
  return vh_operator(h, x_dev, nullptr, nullptr, y_dev, (hipStream_t)stream);
}
extern "C" int cheb_varhelm_apply(void *h, const double *x_dev, double *y_dev, void *stream) { return cheb_varhelm_mult((cheb_varhelm *)h, x_dev, y_dev, stream); }

extern "C" int cheb_varhelm_residual(cheb_varhelm *h, const double *x_dev, const double *f_dev, const double *g_dev, double *out_dev, void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (!f_dev) return chebhip_fail(CHEBHIP_ERR_ARG, "residual: f is NULL");
  int rc = vh_check_vectors(h, "residual", x_dev, f_dev, g_dev, out_dev); if (rc) return rc;
  return vh_operator(h, x_dev, f_dev, g_dev, out_dev, (hipStream_t)stream);
}

extern "C" int cheb_varhelm_precond(void *hv, const double *r_dev, double *z_dev, void *stream) {
  cheb_varhelm *h = (cheb_varhelm *)hv;
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (!r_dev || !z_dev) return chebhip_fail(CHEBHIP_ERR_ARG, "precond: NULL vector");
  if (!h->have_coef) return chebhip_fail(CHEBHIP_ERR_ARG, "cheb_varhelm: set_coefficients has not been called");
  hipStream_t st = (hipStream_t)stream;
  vh_launch_rows(k_vh_over_kappa<1>, k_vh_over_kappa<2>, vh_pairs(h, r_dev, h->tu, nullptr), h, st, r_dev, (const double *)h->kap, h->tu);
  HIP_TRY(hipGetLastError());
  return cheb_helmholtz_solve(h->H, h->tu, z_dev, stream);
}

// solve (q = 0) and solve_deflated on a singular handle (q = its null vectors): b = f - (operator at g)(0), FGMRES, the full grid.
// With q > 0 the system is Pi A x = Pi b in the range of Pi: b, the guess and the result are projected, the operator and the
// preconditioner are the _deflated entries, and the coefficients of the residual b - A x in the null vectors are left in dtot.
static int vh_solve(cheb_varhelm *h, int q, const double *f_dev, const double *g_dev, double *x_dev, int x_nonzero, double *u_full_dev,
                    double rtol, double atol, int max_it, int restart, void *stream) {
  if (restart < 1 || max_it < 0) return chebhip_fail(CHEBHIP_ERR_ARG, "solve: restart = %d, max_it = %d", restart, max_it);
  const long n = (long)h->nf * h->G, nN = (long)h->nf * h->N, nb = (long)h->nf * h->NB;
  if (g_dev && h->NB == 0) return chebhip_fail(CHEBHIP_ERR_ARG, "solve: g given, but every direction is periodic: there is no boundary data");
  if (overlap(x_dev, n, f_dev, n) || (g_dev && overlap(x_dev, n, g_dev, nb))) return chebhip_fail(CHEBHIP_ERR_ARG, "solve: x may not alias f or g");
  if (u_full_dev && (overlap(u_full_dev, nN, f_dev, n) || overlap(u_full_dev, nN, x_dev, n) || (g_dev && overlap(u_full_dev, nN, g_dev, nb))))
    return chebhip_fail(CHEBHIP_ERR_ARG, "solve: u_full may not alias f, g or x");
  if (!q && cheb_helmholtz_singular(h->H))
    return chebhip_fail(CHEBHIP_ERR_ARG, "solve: the problem is singular (c == 0 and every direction periodic or Neumann / Neumann); mult and residual still work");
  if (h->krylov && h->krylov_restart != restart) {          // one pair of bases at a time: at 256^3 and restart 30 they are 8 GB per field
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    chebhip_fgmres_destroy(h->krylov); h->krylov = nullptr; h->krylov_bytes = 0;
  }
  if (!h->krylov) {
    int rc = chebhip_fgmres_create(n, restart, &h->krylov);
    if (rc) { h->krylov = nullptr; return rc; }
    h->krylov_restart = restart;
    h->krylov_bytes = (size_t)(2 * restart + 1) * (size_t)n * sizeof(double);       // the two bases; the rest is O(restart^2)
  }
  chebhip_fgmres *ks = h->krylov;
  int rc = chebhip_fgmres_set_tolerances(ks, rtol, atol, max_it); if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  h->defect_q = 0;
  if ((rc = vh_operator(h, h->zero, f_dev, g_dev, h->bu, st))) return rc;              // b = f - (operator at g)(0): the lift of g
  if (q) {
    if ((rc = vh_remove_null(h, q, h->bu, h->bu, h->ntot, st))) return rc;
    if (x_nonzero && (rc = vh_remove_null(h, q, x_dev, x_dev, h->ntot, st))) return rc;
  }
  rc = chebhip_fgmres_solve(ks, q ? cheb_varhelm_apply_deflated : cheb_varhelm_apply, h, q ? cheb_varhelm_precond_deflated : cheb_varhelm_precond, h,
                            h->bu, x_dev, x_nonzero ? 1 : 0, stream);
  h->iterations = chebhip_fgmres_iterations(ks); h->residual = chebhip_fgmres_residual(ks); h->reason = chebhip_fgmres_reason(ks);
  if (rc) return rc;
  if (q) {
    // the last Pi: the Krylov vectors are in the range of Pi only as far as their roundings allow
    if ((rc = vh_remove_null(h, q, x_dev, x_dev, h->ntot, st))) return rc;
    // what is left of b - A x lies in the null space: its coefficients, from one residual (into the preconditioner's work vector)
    if ((rc = vh_operator(h, x_dev, f_dev, g_dev, h->tu, st)) || (rc = vh_remove_null(h, q, h->tu, nullptr, h->dtot, st))) return rc;
    h->defect_q = q;
  }
  if (u_full_dev) {
    if (h->NB) return helmholtz_extend(h->H, x_dev, g_dev, u_full_dev, stream);
    HIP_TRY(hipMemcpyAsync(u_full_dev, x_dev, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
  }
  return 0;
}

extern "C" int cheb_varhelm_solve(cheb_varhelm *h, const double *f_dev, const double *g_dev, double *x_dev, int x_nonzero, double *u_full_dev,
                                  double rtol, double atol, int max_it, int restart, void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (!f_dev || !x_dev) return chebhip_fail(CHEBHIP_ERR_ARG, "solve: NULL vector");
  if (!h->have_coef) return chebhip_fail(CHEBHIP_ERR_ARG, "cheb_varhelm: set_coefficients has not been called");
  return vh_solve(h, 0, f_dev, g_dev, x_dev, x_nonzero, u_full_dev, rtol, atol, max_it, restart, stream);
}

extern "C" int cheb_varhelm_solve_deflated(cheb_varhelm *h, const double *f_dev, const double *g_dev, double *x_dev, int x_nonzero, double *u_full_dev,
                                           double rtol, double atol, int max_it, int restart, void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (!f_dev || !x_dev) return chebhip_fail(CHEBHIP_ERR_ARG, "solve: NULL vector");
  if (!h->have_coef) return chebhip_fail(CHEBHIP_ERR_ARG, "cheb_varhelm: set_coefficients has not been called");
  const int q = vh_null_count(h, "solve_deflated");
  if (q < 0) return CHEBHIP_ERR_ARG;
  return vh_solve(h, q, f_dev, g_dev, x_dev, x_nonzero, u_full_dev, rtol, atol, max_it, restart, stream);
}

// Pi of in (in == out allowed); the identity on a nonsingular handle
extern "C" int cheb_varhelm_remove_null(cheb_varhelm *h, const double *in_dev, double *out_dev, void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (!in_dev || !out_dev) return chebhip_fail(CHEBHIP_ERR_ARG, "remove_null: NULL vector");
  if (!h->have_coef) return chebhip_fail(CHEBHIP_ERR_ARG, "cheb_varhelm: set_coefficients has not been called");
  const long n = (long)h->nf * h->G;
  if (in_dev != out_dev && overlap(in_dev, n, out_dev, n)) return chebhip_fail(CHEBHIP_ERR_ARG, "remove_null: out may be in itself, but may not overlap it otherwise");
  const int q = vh_null_count(h, "remove_null");
  if (q < 0) return CHEBHIP_ERR_ARG;
  if (q) return vh_remove_null(h, q, in_dev, out_dev, h->ntot, (hipStream_t)stream);
  if (in_dev != out_dev) HIP_TRY(hipMemcpyAsync(out_dev, in_dev, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

extern "C" int cheb_varhelm_apply_deflated(void *hv, const double *x_dev, double *y_dev, void *stream) {
  int rc = cheb_varhelm_apply(hv, x_dev, y_dev, stream); if (rc) return rc;
  return cheb_varhelm_remove_null((cheb_varhelm *)hv, y_dev, y_dev, stream);
}
extern "C" int cheb_varhelm_precond_deflated(void *hv, const double *r_dev, double *z_dev, void *stream) {
  int rc = cheb_varhelm_precond(hv, r_dev, z_dev, stream); if (rc) return rc;
  return cheb_varhelm_remove_null((cheb_varhelm *)hv, z_dev, z_dev, stream);
}

extern "C" int cheb_varhelm_null_count(const cheb_varhelm *h) {
  if (!h || !h->have_coef) return -1;
  if (!cheb_helmholtz_singular(h->H)) return 0;
  return h->null.m > 3 ? -1 : 1 << h->null.m;
}

// lambda = N^T (b - A x) / G of the last deflated solve: nfields x q values, field by field
extern "C" int cheb_varhelm_defect(cheb_varhelm *h, double *out) {
  if (!h || !out) return chebhip_fail(CHEBHIP_ERR_ARG, "defect: NULL argument");
  if (!h->defect_q) return chebhip_fail(CHEBHIP_ERR_ARG, "defect: no deflated solve of a singular problem has run on this handle");
  std::vector<double> tot((size_t)h->nf * VH_TS);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(tot.data(), h->dtot, tot.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int f = 0; f < h->nf; f++)
    for (int j = 0; j < h->defect_q; j++) out[(size_t)f * h->defect_q + j] = tot[(size_t)f * VH_TS + 8 + j];
  return 0;
}

// The null vectors of a geometry whose every direction is periodic or Neumann / Neumann: flags[j], j < q, has bit k set where
// vector j alternates ((-1)^index) in direction k; flags[0] = 0 is the constant.  Returns q = 2^(even periodic directions), or
// -CHEBHIP_ERR_* with the error set (more than three such directions among them).  Host only.
extern "C" int cheb_varhelm_null_signs_host(int d, const int *dims, const int *basis, int *flags) {
  if (!dims || !flags || d < 1 || d > VMAXD) return -chebhip_fail(CHEBHIP_ERR_ARG, "null_signs: d = %d must be in 1..10 and dims, flags given", d);
  for (int k = 0; k < d; k++) if (dims[k] < 1) return -chebhip_fail(CHEBHIP_ERR_ARG, "null_signs: dims[%d] = %d", k, dims[k]);
  int dir[3];
  const int m = vh_even_periodic(d, dims, basis, dir);
  if (m > 3) return -chebhip_fail(CHEBHIP_ERR_ARG, "null_signs: %d even periodic directions give %ld null vectors: more than three such directions (8 vectors) are not supported", m, 1L << m);
  for (int j = 0; j < (1 << m); j++) {
    flags[j] = 0;
    for (int b = 0; b < m; b++) if (j >> b & 1) flags[j] |= 1 << dir[b];
  }
  return 1 << m;
}

extern "C" int cheb_varhelm_iterations(const cheb_varhelm *h) { return h ? h->iterations : -1; }
extern "C" double cheb_varhelm_last_residual(const cheb_varhelm *h) { return h ? h->residual : -1.0; }
extern "C" int cheb_varhelm_reason(const cheb_varhelm *h) { return h ? h->reason : 0; }
