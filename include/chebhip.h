/*
 * chebhip.h -- C ABI of libchebhip.so: the MI355X (gfx950) implementation of
 * the matrix-free Chebyshev spectral operator apply of jedbrown/spectral-petsc.
 *
 * This is the drop-in boundary.  Each entry point names the reference
 * interface it replaces (file:line relative to the reference tree).  The
 * PETSc-level symbols of chebyshev.h:27-34 (MatCreateCheb / ChebMult /
 * ChebDestroy ...) are a thin adapter over these calls: see
 * adapter/chebyshev_petsc.c and INTEGRATION.md.
 *
 * Conventions
 *  - all data IEEE float64; tensors row-major, LAST listed dim fastest
 *    (chebyshev.c:107-120); grid index i along a dim is x_i = cos(i pi/(P-1)).
 *  - *_dev pointers are device (HBM) pointers; `stream` is a hipStream_t passed
 *    as void* (NULL = default stream).  Device-pointer calls are asynchronous
 *    on that stream; *_host calls stage through device memory and return after
 *    the result is in the host buffer.  A stream created with
 *    hipStreamNonBlocking is fine: state the library allocates on first use is
 *    complete before the call that allocates it enqueues anything.  The set_* /
 *    create / update calls that take host data are synchronous copies that do
 *    NOT wait for work still queued on a non-blocking stream: synchronise that
 *    stream before changing the state a queued call reads (as before VecSet on
 *    a vector a MatMult in flight is reading).
 *  - every call returns 0 on success or a CHEBHIP_ERR_* code; nothing throws or
 *    exits across the ABI.  chebhip_last_error() returns a message for the
 *    calling thread's most recent failure.
 *  - a handle may be used from one host thread at a time (the reference's ctx
 *    is likewise non-reentrant: one mutable work buffer, chebyshev.h:23).
 *  - there is NO CPU fallback: without a usable HIP device the create calls
 *    fail with CHEBHIP_ERR_DEVICE.
 */
#ifndef CHEBHIP_H
#define CHEBHIP_H

#ifdef __cplusplus
extern "C" {
#endif

enum {
  CHEBHIP_OK = 0,
  CHEBHIP_ERR_SIZE = 1,     /* n < 2              (chebyshev.c:18,98)  -> PETSC_ERR_USER */
  CHEBHIP_ERR_TDIM = 2,     /* tr out of range    (chebyshev.c:106)    -> PETSC_ERR_USER */
  CHEBHIP_ERR_DIMS = 3,     /* bad dims / product (chebyshev.c:122)    -> PETSC_ERR_USER */
  CHEBHIP_ERR_ARG = 4,      /* NULL handle/pointer, unsupported value  -> PETSC_ERR_ARG_WRONG */
  CHEBHIP_ERR_DEVICE = 5,   /* HIP runtime failure / no device         -> PETSC_ERR_LIB */
  CHEBHIP_ERR_MEMORY = 6    /* allocation failure                      -> PETSC_ERR_MEM */
};

const char *chebhip_last_error(void);
/* Library/ABI version (major*100 + minor) and the offload arch it was built for. */
int chebhip_version(void);
const char *chebhip_arch(void);

/* A linear map on device vectors: y = A x.  ell_op_mult, stokes_op_mult and stokes_op_mult_vv have
 * exactly this shape (ctx = the operator handle) and can be passed as is. */
typedef int (*chebhip_apply_fn)(void *ctx, const double *x_dev, double *y_dev, void *stream);
/* Sums `count` device doubles over the ranks in place, ordered on `stream` (ncclAllReduce of a few doubles per
 * Krylov iteration): what a multi-rank host gives the solvers below. */
typedef int (*chebhip_reduce_fn)(void *ctx, double *vals_dev, int count, void *stream);

/* ------------------------------------------------------------------------- */
/* Kernel level: the N-D Chebyshev derivative (chebyshev.h:18-24,31-34).      */
/* ------------------------------------------------------------------------- */
typedef struct cheb_plan cheb_plan;

/* Replaces MatCreateCheb (chebyshev.c:89-138) and, for rank 1, MatCreateChebD1
 * (chebyshev.c:8-33).  dims is copied.  Errors as chebyshev.c:98,106,122. */
int cheb_plan_create(int rank, int tr, const int *dims, cheb_plan **out);

/* Replaces ChebMult (chebyshev.c:142-199) / ChebD1Mult (:37-71):
 * y = d/dx_tr x.  x and y are distinct N-element arrays, x is not modified. */
int cheb_apply(cheb_plan *plan, const double *x_dev, double *y_dev, void *stream);
int cheb_apply_host(cheb_plan *plan, const double *x_host, double *y_host);

/* Replaces ChebDestroy (chebyshev.c:223-235) / ChebD1Destroy (:75-85). */
int cheb_plan_destroy(cheb_plan *plan);

/* Number of elements N = prod(dims) the plan was created for. */
long cheb_plan_size(const cheb_plan *plan);

/* Slab / pencil building block for the multi-GPU path (no counterpart in the serial reference):
 * a plan on a tensor that stores only the INTERIOR points of every line along `tr`
 * (dims[tr] = P-2; the end points are implicit zeros) -- the layout of the reference's global
 * vectors (SetupBC, elliptic.C:372-434) and of any slab cut from them along another dim. */
int cheb_plan_create_trimmed(int rank, int tr, const int *dims, cheb_plan **out);
/* y = acc + alpha * (D_tr D_tr x) at the stored points: one direction of the linear
 * MatMult_Elliptic (elliptic.C:309-334 with eta = 1, deta = 0).  acc may be NULL, or alias y. */
int cheb_apply_lap1d(cheb_plan *plan, const double *x_dev, const double *acc_dev, double alpha,
                     double *y_dev, void *stream);
/* Copies between a slab (m0, M1, R) row-major and the buffer an all-to-all moves: for every peer s the
 * block slab[:, c1[s]:c1[s+1], :] contiguously, blocks in rank order (c1: G+1 host values, 0 .. M1).
 * pack: buf <- slab (before the forward transpose).  unpack_add: out = acc + alpha * slab-ordered(buf)
 * (after the backward transpose; acc may be NULL or alias out). */
int cheb_slab_pack(long m0, long M1, long R, int G, const long *c1_host, const double *slab_dev,
                   double *buf_dev, void *stream);
int cheb_slab_unpack_add(long m0, long M1, long R, int G, const long *c1_host, const double *buf_dev,
                         const double *acc_dev, double alpha, double *out_dev, void *stream);

/* ------------------------------------------------------------------------- */
/* Resampling: moves a field between two Chebyshev-Gauss-Lobatto grids (no    */
/* counterpart in the reference; the interpolation PETSc's                    */
/* -snes_grid_sequence needs between levels).  Tensors are row-major with     */
/* ncomp components innermost (node-major, as the Stokes velocity).  Per      */
/* direction a grid of n points has two node sets:                            */
/*   CHEB_NODES_ALL       x_j = cos(pi j/(n-1)), j = 0 .. n-1 (n values)      */
/*   CHEB_NODES_INTERIOR  the points j = 1 .. n-2 of that grid (n-2 values):  */
/*                        the global-vector layout of the MatShells and the   */
/*                        node set of the Stokes pressure                     */
/* ------------------------------------------------------------------------- */
typedef struct cheb_resample cheb_resample;
enum { CHEB_NODES_ALL = 0, CHEB_NODES_INTERIOR = 1 };

/* y = (R_0 (x) ... (x) R_{d-1}) x, R_k the Lagrange interpolation matrix from the input to the output node set of direction k.
 * 1 <= d <= 10; 2 <= dims[k] <= 1024 (3 for INTERIOR); 1 <= ncomp <= 4; fewer than 2^31 values on either side.  dims are copied;
 * the matrices are built in long double at create (barycentric form; an output node that is an input node gets an exact unit
 * row, so equal grids copy their input and coarse values are injected unchanged into a finer grid containing their nodes).
 * The handle owns its matrices and two work buffers: apply allocates nothing and does not synchronise the host. */
int  cheb_resample_create(int d, const int *dims_in, int nodes_in, const int *dims_out, int nodes_out,
                          int ncomp, cheb_resample **out);
/* x: cheb_resample_size(r, 0) values, y: cheb_resample_size(r, 1) values; x and y must not overlap.  Asynchronous on `stream`. */
int  cheb_resample_apply(cheb_resample *r, const double *x_dev, double *y_dev, void *stream);
int  cheb_resample_destroy(cheb_resample *r);
long cheb_resample_size(const cheb_resample *r, int which);           /* 0: input values, 1: output values; -1 on a bad argument */
/* The (stored n_out) x (stored n_in) matrix of one direction, row-major, into a HOST buffer; needs no device. */
int  cheb_resample_matrix_host(int n_in, int nodes_in, int n_out, int nodes_out, double *R);

/* ------------------------------------------------------------------------- */
/* The modal side of the Chebyshev-Gauss-Lobatto grids (the reference's       */
/* ChebMult goes values -> DCT -> recurrence -> DCT, chebyshev.c:142-199, but */
/* never hands the coefficients out): coefficient transforms, modal filters,  */
/* per-direction spectra and Clenshaw-Curtis quadrature.  Per direction of    */
/* n points, N = n - 1, x_j = cos(pi j / N), c_0 = c_N = 2, otherwise c = 1:  */
/*   backward  B[j][k] = T_k(x_j) = cos(pi j k / N)    coefficients -> values */
/*   forward   T[k][j] = 2 / (N c_k c_j) cos(pi j k / N)          B T = I     */
/*   weights   w = I^T T, I_k = 2 / (1 - k^2) (k even), 0 (k odd): exact for  */
/*             polynomials of degree <= N, sum w = 2                          */
/*   filter    F = B diag(sigma_0 .. sigma_N) T                               */
/* all built in long double and rounded once.  Fields are `nfields` arrays of */
/* prod(dims) values, field-major and row-major over ALL nodes (the layout of */
/* cheb_helmholtz_solve_bc's full-grid arrays); coefficient arrays have the   */
/* same shape, entry (k_0, .., k_{d-1}) multiplying T_{k_0}(x) T_{k_1}(y) ... */
/* ------------------------------------------------------------------------- */
typedef struct cheb_modal cheb_modal;

/* 1 <= d <= 10; 2 <= dims[k] <= 1024; 1 <= nfields <= 16; fewer than 2^31 values.  The handle owns its matrices, two work buffers
 * and the scratch of the reductions: the calls below allocate nothing and do not synchronise the host. */
int  cheb_modal_create(int d, const int *dims, int nfields, cheb_modal **out);
int  cheb_modal_destroy(cheb_modal *h);
long cheb_modal_size(const cheb_modal *h);                 /* nfields * prod(dims); -1: NULL */
long cheb_modal_spectrum_size(const cheb_modal *h);        /* nfields * sum(dims); -1: NULL */
/* a = (T_0 (x) .. (x) T_{d-1}) u and u = (B_0 (x) .. (x) B_{d-1}) a: one launch per direction.  Input and output must not overlap. */
int  cheb_modal_forward (cheb_modal *h, const double *u_dev, double *a_dev, void *stream);
int  cheb_modal_backward(cheb_modal *h, const double *a_dev, double *u_dev, void *stream);
/* sigma of direction k: dims[k] HOST values; NULL clears.  Synchronous (see the conventions above). */
int  cheb_modal_set_filter(cheb_modal *h, int k, const double *sigma_host);
/* v = (F_0 (x) .. (x) F_{d-1}) u.  A direction whose sigma is unset or all ones is dropped (the values keep their bits along it);
 * with no direction left this is a copy.  u and v must not overlap. */
int  cheb_modal_filter  (cheb_modal *h, const double *u_dev, double *v_dev, void *stream);
/* E[f][k][m] = sum of a^2 over every index except direction k's, held at m: field by field, direction by direction, dims[k] values
 * each (cheb_modal_spectrum_size doubles). */
int  cheb_modal_spectrum(cheb_modal *h, const double *a_dev, double *E_dev, void *stream);
/* out[f] = sum_i W_i u_i, or sum_i W_i u_i v_i when v_dev is not NULL (u == v is allowed), W_i = prod_k w_k[i_k]: nfields DEVICE
 * values.  spectrum and integrate add in a fixed order: the same input gives the same bits on every run. */
int  cheb_modal_integrate(cheb_modal *h, const double *u_dev, const double *v_dev, double *out_dev, void *stream);
/* Host-side builders; they need no device.  n x n row-major (which = 0: T, 1: B), n weights, and F for n values of sigma
 * (all ones: exactly the identity). */
int  cheb_modal_matrix_host(int n, int which, double *M);
int  cheb_modal_weights_host(int n, double *w);
int  cheb_modal_filter_matrix_host(int n, const double *sigma, double *F);

/* ------------------------------------------------------------------------- */
/* Evaluation at arbitrary points of the reference cube [-1, 1]^d (no         */
/* counterpart in the reference): probes, line and plane cuts, plotting grids */
/* and tracer positions that live on the device.  Fields use the full-grid,   */
/* field-major layout of cheb_modal_*.  Per direction of n points, N = n - 1, */
/* x_j = cos(pi j / N) (index 0 is x = +1), barycentric weights w_j = (-1)^j, */
/* halved at j = 0 and j = N; the row of a coordinate x is                    */
/*   l_j(x) = (w_j / (x - x_j)) / sum_k w_k / (x - x_k)                       */
/* evaluated in the nearest-node form, which cannot overflow: s = the node    */
/* nearest to x, d_j = x - x_j, r_s = 1, r_j = (w_j / w_s) (d_s / d_j),       */
/* l = r / sum r.  d_s == 0 gives the exact unit row e_s (a point on a node   */
/* returns the field's own bits); a NaN or infinite coordinate gives NaN for  */
/* that point only; |x| > 1 is EXTRAPOLATED by the same formula, not clamped  */
/* (the interpolant grows like T_N outside the cube).  The sums run in an     */
/* order that depends on the shape alone: results repeat bit for bit.         */
/* ------------------------------------------------------------------------- */
typedef struct cheb_points cheb_points;

/* 1 <= d <= 10; 2 <= dims[k] <= 1024; 1 <= nfields <= 16; fewer than 2^31 values.  The handle owns the node tables (long double,
 * rounded once, shared by equal extents) and the work memory of one chunk of cheb_points_chunk points -- the rows and direction
 * 0's output, at most max(bytes of the fields, 32 MiB): cheb_points_rows and cheb_points_eval allocate nothing and do not
 * synchronise the host. */
int  cheb_points_create(int d, const int *dims, int nfields, cheb_points **out);
int  cheb_points_destroy(cheb_points *h);
long cheb_points_chunk(const cheb_points *h);              /* points per chunk: a multiple of 64 where memory allows, <= 1024; -1: NULL */
/* R[i][j] = l_j(x[i]) of direction k: m x dims[k] DEVICE values, row-major, from m DEVICE coordinates. */
int  cheb_points_rows(cheb_points *h, int k, const double *x_dev, long m, double *R_dev, void *stream);
/* out[f][p] = sum l_{i0}(xi[p][0]) .. l_{i(d-1)}(xi[p][d-1]) u[f][i0 .. i(d-1)]: xi is npts x d (point-major), out nfields x npts.
 * Per chunk: the rows, direction 0 as one line product on the FP64 matrix cores, one contraction per (field, point).
 * npts = 0 is a no-op; out must not overlap u. */
int  cheb_points_eval(cheb_points *h, const double *u_dev, const double *xi_dev, long npts, double *out_dev, void *stream);
/* The transpose of cheb_points_eval: out[f][i0 .. i(d-1)] = sum_p s[f][p] l_{i0}(xi[p][0]) .. l_{i(d-1)}(xi[p][d-1]) -- point forces,
 * point sources, the transpose of an observation operator.  s is nfields x npts (the layout eval writes), xi npts x d (the layout
 * eval reads), out `nfields` stacked full-grid fields.  Points run in passes of cheb_points_spread_pass: the rows of all
 * directions into the handle's work memory, then one product on the FP64 matrix cores whose contracted index is the point and
 * whose second operand, ((s l_1) l_2 ..) l_{d-1}, is formed on chip.  The first pass stores (or adds, CHEB_SPREAD_ACCUMULATE: out +=
 * ..), later passes add; no atomics, and the order of the additions depends on (dims, nfields, npts, pass size) alone: results
 * repeat bit for bit.  CHEB_SPREAD_DELTA divides the result at node i by the Clenshaw-Curtis weights w_{i0} .. w_{i(d-1)} (by
 * multiplying with the inverses of cheb_modal_weights_host's values, long double, rounded once; built and uploaded by the first
 * such call, which therefore allocates and synchronises once): cheb_modal_integrate(out, phi) then equals sum_p s_p phi(x_p) for
 * every polynomial phi of the grid -- a point source of strength s.  Otherwise the call allocates nothing and does not
 * synchronise the host.  A point on a node has a unit row: spreading one such point stores s at that node bit for bit and zeros
 * elsewhere.  A NaN or infinite coordinate makes every field's output NaN (the rows are shared), a NaN strength s[f][p] field f's
 * only; |x| > 1 extrapolates as in eval.  npts = 0 zero-fills out, or leaves it alone with CHEB_SPREAD_ACCUMULATE; out must not
 * overlap s or xi. */
enum { CHEB_SPREAD_ACCUMULATE = 1, CHEB_SPREAD_DELTA = 2 };
int  cheb_points_spread(cheb_points *h, const double *s_dev, const double *xi_dev, long npts, double *out_dev, int flags, void *stream);
/* points per pass of cheb_points_spread: as many as the handle's work memory holds rows for, whole chunks of 16, at most the
 * option points_spread_pass where that is set; -1: NULL */
long cheb_points_spread_pass(const cheb_points *h);
/* Tensor grids of arbitrary coordinates: direction k takes m[k] coordinates (HOST counts), the DEVICE array `coords` holds them
 * direction after direction (sum of m[k] values); out is nfields x m[0] x .. x m[d-1], field-major and row-major.  One line
 * product per direction, shrinking directions first.  A plane cut is m[k] = 1, a line cut has d - 1 of them.
 * cheb_points_grid_reserve (synchronous, d HOST ints >= 1) allocates the rows and the two intermediates for every grid with
 * m[k] <= m_max[k]; cheb_points_eval_grid allocates nothing and refuses a larger grid (CHEBHIP_ERR_ARG).  A count of 0 is a no-op. */
int  cheb_points_grid_reserve(cheb_points *h, const int *m_max);
int  cheb_points_eval_grid(cheb_points *h, const double *u_dev, const double *coords_dev, const int *m, double *out_dev, void *stream);
/* Host-side twins; they need no device.  The n nodes, and the m x n rows (row-major) of m HOST coordinates by the same formula in
 * long double on the DOUBLE node table, rounded once. */
int  cheb_nodes_host(int n, double *x);
int  cheb_points_matrix_host(int n, int m, const double *x_host, double *R);
/* First derivatives at points.  The derivative of the interpolant is another row per direction: with c_j = w_j / w_s,
 * q_j = c_j / d_j and r_j = q_j d_s (j != s), R = 1 + sum r_j, Q2 = sum q_k / d_k, T = sum q_k (x_s - x_k) / d_k (sums over k != s),
 *   l'_j(x) = (q_j / R) ((1 + d_s^2 Q2) / R - d_s / d_j)  (j != s),    l'_s(x) = -T / R^2,
 * the exact derivative of the rational function the value rows evaluate on the rounded nodes.  Nothing divides by d_s: a point on
 * a node gets l'_j = q_j, l'_s = -sum q_k, a row of the differentiation matrix, by the same instructions.  A NaN or infinite
 * coordinate gives a row of NaN, |x| > 1 extrapolates.  cheb_points_drows: R[i][j] = l'_j(x[i]) of direction k, m x dims[k] DEVICE
 * values (k_points_rows writing derivative rows: the lane groups, reductions and order of its value rows); cheb_points_dmatrix_host is its host twin, long
 * double on the DOUBLE node table, rounded once. */
int  cheb_points_drows(cheb_points *h, int k, const double *x_dev, long m, double *R_dev, void *stream);
int  cheb_points_dmatrix_host(int n, int m, const double *x_host, double *R);
/* cheb_points_eval, cheb_points_spread and cheb_points_eval_grid with the rows of the directions flagged in `deriv` exchanged for
 * their derivative rows: d HOST ints, each 0 or 1 (anything else: CHEBHIP_ERR_ARG), so (1, 0, 0) is d/dx_0 and (1, 1, 0) the mixed
 * derivative; pure second derivatives are not offered.  The line products, contractions, chunks and passes are those of the plain
 * calls; NULL or all zeros runs the plain call's launches and gives its bits.  With CHEB_SPREAD_DELTA cheb_modal_integrate(out,
 * phi) is sum_p s_p d^alpha phi(x_p): a force dipole, the transpose of a gradient observation.  Derivatives are with respect to
 * the reference coordinates; a box of length L_k takes the factor 2 / L_k per flagged direction. */
int  cheb_points_eval_deriv(cheb_points *h, const double *u_dev, const double *xi_dev, long npts, const int *deriv, double *out_dev,
                            void *stream);
int  cheb_points_spread_deriv(cheb_points *h, const double *s_dev, const double *xi_dev, long npts, const int *deriv, double *out_dev,
                              int flags, void *stream);
int  cheb_points_eval_grid_deriv(cheb_points *h, const double *u_dev, const double *coords_dev, const int *m, const int *deriv,
                                 double *out_dev, void *stream);
/* The gradient in one call: out[f][c][p] = s_c d u_f / d x_c (xi[p]), c = 0 .. d-1, out nfields x d x npts; with
 * CHEB_POINTS_GRAD_VALUE out is nfields x (d + 1) x npts and component c = d holds the value, so a derivative's index does not
 * depend on the flag.  scale: d finite HOST values s_k = 2 / L_k as in cheb_grad_create, NULL = ones; one multiplication at the
 * store.  Per chunk of cheb_points_chunk / 2 points (the handle's work memory as created): k_points_rows writes both row sets,
 * ONE direction-0 line product over the stacked value and derivative rows gives every point a value block and a derivative
 * block, and k_points_contract in its gradient form walks the value block once for the value and every direction >= 1 and the derivative block
 * once for direction 0, a workgroup per (field, point) and block.  d = 1: the line product's two outputs are the result.  Where the
 * work memory holds a single point, a point takes one pass of the eval pipeline per component.  No atomics, results repeat bit for
 * bit; the call allocates nothing and does not synchronise the host.  npts = 0 is a no-op; out must not overlap u. */
enum { CHEB_POINTS_GRAD_VALUE = 1 };
int  cheb_points_eval_grad(cheb_points *h, const double *u_dev, const double *xi_dev, long npts, const double *scale_host, int flags,
                           double *out_dev, void *stream);

/* ------------------------------------------------------------------------- */
/* Dealiased products and advection terms (no counterpart in the reference):  */
/* the nonlinear terms of the explicit side of a time-dependent problem.  The */
/* nodal product of two degree-N interpolants has degree 2N and its upper     */
/* half folds back onto the retained modes (u = T_N: the nodal square is 1,   */
/* the truncation of T_N^2 = (T_0 + T_2N) / 2 is 1/2).  Per direction of n    */
/* coarse points (N = n - 1) and m >= n fine points (M = m - 1):              */
/*   R (m x n)  Lagrange interpolation coarse -> fine nodes: the matrix of    */
/*              cheb_resample_matrix_host(n, ALL, m, ALL), bit for bit        */
/*   P (n x m)  = B_n T_m[0:n, :]: fine values -> fine coefficients, modes    */
/*              0 .. N kept and evaluated at the coarse nodes (m == n: I)     */
/*   G (m x n)  = R D_n: differentiate on the coarse grid and interpolate     */
/* built in long double and rounded once.  For M > 3N/2                       */
/*   (P_0 (x) ..) (((R_0 (x) ..) u) o ((R_0 (x) ..) v))                       */
/* is exactly the truncation to degree N per direction of the polynomial      */
/* product (the aliases of the modes k > M land at 2M - k > N); the smallest  */
/* such m is ceil(3n/2), the default.  Fields use the full-grid, field-major  */
/* layout of cheb_modal_*.                                                    */
/* ------------------------------------------------------------------------- */
typedef struct cheb_dealias cheb_dealias;

/* ceil(3n/2) for 2 <= n <= 1024, -1 otherwise; and R, P or G (which = 0, 1, 2) of n coarse and m >= n fine points, row-major, into
 * a HOST buffer of n m doubles.  Neither needs a device. */
int  cheb_dealias_fine_size(int n);
int  cheb_dealias_matrix_host(int n, int m, int which, double *A);
/* 1 <= d <= 10; 2 <= dims[k] <= 1024; 1 <= nfields <= 16; dims_fine NULL: the 3/2 rule (n <= 682), otherwise dims[k] <= dims_fine[k]
 * <= 1024 (equal: that direction runs unpadded); every array the handle touches holds fewer than 2^31 values.  The handle owns its
 * matrices and work memory -- the product on the fine grid (nfields prod(m) values: the only array of that size, no operand ever
 * exists on the fine grid) and the operands taken to the fine grid in every direction but one; cheb_dealias_work_bytes reports
 * it.  multiply and advect allocate nothing and do not synchronise the host; outputs must not overlap inputs. */
int  cheb_dealias_create(int d, const int *dims, const int *dims_fine, int nfields, cheb_dealias **out);
int  cheb_dealias_destroy(cheb_dealias *h);
int  cheb_dealias_fine_dims(const cheb_dealias *h, int *dims_fine);     /* d HOST ints */
long cheb_dealias_size(const cheb_dealias *h);                          /* nfields * prod(dims); -1: NULL */
long cheb_dealias_work_bytes(const cheb_dealias *h);                    /* device bytes the handle owns now; -1: NULL */
/* out[f] = Pi_N (u[f] v[f]), f < nfields; u == v is allowed (squares). */
int  cheb_dealias_multiply(cheb_dealias *h, const double *u_dev, const double *v_dev, double *out_dev, void *stream);
/* out[f] = Pi_N (sum_k vel[k] d_k c[f]): vel holds d fields, c and out nfields.  Its work memory (the d (1 + nfields) operand
 * images) is allocated by cheb_dealias_reserve_advect (synchronous); without it advect returns CHEBHIP_ERR_ARG. */
int  cheb_dealias_reserve_advect(cheb_dealias *h);
int  cheb_dealias_advect(cheb_dealias *h, const double *vel_dev, const double *c_dev, double *out_dev, void *stream);

/* ------------------------------------------------------------------------- */
/* Partial contractions (no counterpart in the reference): the numbers a run  */
/* is made for -- mean profiles, plane-averaged fluxes <w T>(z), the flux     */
/* through a wall, the value or normal derivative of a field on a face, a     */
/* marginal of a density.  A SUBSET of the directions of u, or of the product */
/* u v, is summed against one weight vector per contracted direction:         */
/*   out[f][kept indices] = sum over the contracted indices of                */
/*                          prod_{k contracted} w_k[i_k] u[f][i] (v[f][i])    */
/* with the kept indices row-major in the original order of the directions.   */
/* Fields use the full-grid, field-major layout of cheb_modal_*.  Contracting */
/* every direction with the default weights is cheb_modal_integrate.  The     */
/* weight vectors of one direction of n points (index 0 is x = +1):           */
/*   CHEB_W_INTEGRAL     the Clenshaw-Curtis weights (cheb_modal_weights_host)*/
/*   CHEB_W_MEAN         half of them: the mean over [-1, 1]                  */
/*   CHEB_W_NODE   j     e_j: the value on the grid plane i_k = j             */
/*   CHEB_W_DNODE  j     row j of D_n: d/dx_k on that plane.  The OUTWARD     */
/*                       derivative is + this at j = 0 and - this at j = n-1  */
/*                       (the convention of cheb_helmholtz_create_bc); the    */
/*                       sign is the caller's                                 */
/*   CHEB_W_POINT  x     the barycentric row of cheb_points_matrix_host: the  */
/*                       value on the plane x_k = x                           */
/*   CHEB_W_DPOINT x     r(x)^T D_n: d/dx_k on the plane x_k = x              */
/* built in long double and rounded once.  No atomics: the additions run in   */
/* an order that depends on (dims, nfields, contract) alone, so results       */
/* repeat bit for bit, and an output reads only the values it owns (a NaN in  */
/* u stays in its own outputs).  With T terms per output over S contracted    */
/* directions every output is within (T + S + 4) 2^-53 sum |W_i u_i v_i| of   */
/* the exact sum with the weights as uploaded.                                */
/* ------------------------------------------------------------------------- */
typedef struct cheb_reduce cheb_reduce;
enum { CHEB_W_INTEGRAL = 0, CHEB_W_MEAN = 1, CHEB_W_NODE = 2, CHEB_W_DNODE = 3, CHEB_W_POINT = 4, CHEB_W_DPOINT = 5 };

/* n HOST values; arg is the node index j or the coordinate x (ignored by INTEGRAL and MEAN).  A j that is no index of the line or
 * an unknown kind is CHEBHIP_ERR_ARG; a NaN or infinite x gives a row of NaN.  Needs no device. */
int  cheb_reduce_weights_host(int n, int kind, double arg, double *w);
/* 1 <= d <= 10; 2 <= dims[k] <= 1024; 1 <= nfields <= 16; fewer than 2^31 input values; contract: d flags, at least one of them
 * nonzero (CHEBHIP_ERR_ARG otherwise).  Contracted directions start with CHEB_W_INTEGRAL.  The handle owns its weights and the
 * scratch of the partial sums: cheb_reduce_apply allocates nothing and does not synchronise the host. */
int  cheb_reduce_create(int d, const int *dims, int nfields, const int *contract, cheb_reduce **out);
int  cheb_reduce_destroy(cheb_reduce *h);
/* The weights of the contracted direction k: dims[k] HOST values, NULL restores the default; a kept direction is CHEBHIP_ERR_ARG.
 * Synchronous, like cheb_modal_set_filter. */
int  cheb_reduce_set_weights(cheb_reduce *h, int k, const double *w_host);
long cheb_reduce_size(const cheb_reduce *h, int which);    /* 0: input values nfields * prod(dims), 1: output values; -1 on a bad argument */
int  cheb_reduce_slices(const cheb_reduce *h);             /* partial sums per output value (1: stored directly, no fold launch); -1: NULL */
/* v_dev NULL: the contraction of u; otherwise of u v (u == v is allowed).  out: cheb_reduce_size(h, 1) DEVICE values, field-major;
 * it must not overlap u or v. */
int  cheb_reduce_apply(cheb_reduce *h, const double *u_dev, const double *v_dev, double *out_dev, void *stream);

/* ------------------------------------------------------------------------- */
/* Field statistics (no counterpart in the reference): what is asked of a     */
/* field after every step and is no weighted sum -- extrema and where they    */
/* are, the NaN count, weighted moments; volume-weighted histograms and       */
/* conditional sums; the advective stability number.  Fields use the          */
/* full-grid, field-major layout of cheb_modal_*.  The weight of a node is    */
/* W_i = prod_k w_k[i_k]; every direction starts with the Clenshaw-Curtis     */
/* weights (cheb_modal_weights_host), so a mass is a volume of [-1, 1]^d:     */
/* all ones turns masses into node counts, CC L_k / 2 gives physical volume.  */
/* No atomics: the order of every addition and the launch geometry depend on  */
/* (dims, nfields, nbins, mode) alone, so results repeat bit for bit, on any  */
/* stream; a field's results read only that field's values (a NaN or Inf in   */
/* field f leaves every other field's output as it was).  With U = 2^-53, T   */
/* values per field and the weights as uploaded:                              */
/*   |M_p - exact|  <= (T + d + p + 4) U sum_i |W_i| |u_i - c|^p              */
/*   |mass - exact| <= (T_b + d + 3) U sum_{i in slot} |W_i c_i|, T_b = the   */
/*                     count of the slot; exactly +0.0 for T_b = 0            */
/*   cfl: within (d + 2) U relative of the exact sum at the reported node,    */
/*        which no other node's exact sum exceeds by more than that           */
/* and counts, slots, min, max, indices and the NaN count are exact.          */
/* ------------------------------------------------------------------------- */
typedef struct cheb_stats cheb_stats;
enum { CHEB_STATS_UNIFORM = 0, CHEB_STATS_EDGES = 1 };

/* h[j] = the smaller of the distances from node j of n CGL nodes to its neighbours (the one distance there is at j = 0 and n - 1),
 * and r[j] = s / h[j]: long double (the gap between two nodes as a product of two sines, their arguments reduced in integers),
 * rounded once.  2 <= n <= 1024; a NaN s is CHEBHIP_ERR_ARG.  They need no device. */
int  cheb_stats_spacing_host(int n, double *h);
int  cheb_stats_rate_host(int n, double s, double *r);
/* The checks of cheb_stats_create and of nbins, without a handle: 0 or the error cheb_stats_create / cheb_stats_histogram would
 * return.  1 <= d <= 10 (CHEBHIP_ERR_ARG otherwise); 2 <= dims[k] <= 1024; 1 <= nfields <= 16; 1 <= nbins <= max_bins <= 1024;
 * fewer than 2^31 input values.  Needs no device. */
int  cheb_stats_check(int d, const int *dims, int nfields, int max_bins, int nbins);
/* The handle owns the weight vectors, the rates of cfl, the partial results of the workgroups and those of the histogram for
 * max_bins bins: the compute calls below allocate nothing and do not synchronise the host (but see cheb_stats_cfl).  The
 * partial results and the rates are one set per handle, so a handle is used from ONE stream at a time: a call on another stream
 * must be ordered after the handle's earlier calls by the caller (an event or a synchronise), as for any buffer they share. */
int  cheb_stats_create(int d, const int *dims, int nfields, int max_bins, cheb_stats **out);
int  cheb_stats_destroy(cheb_stats *h);
/* The weights of direction k: dims[k] HOST values, NULL restores the default.  Synchronous, like cheb_reduce_set_weights. */
int  cheb_stats_set_weights(cheb_stats *h, int k, const double *w_host);
/* 0: input values nfields * prod(dims); 1: values of a summary, 9 * nfields; 2: max_bins; 3, 4: workgroups per field of summary /
 * cfl and of histogram (how many partial results the folds add); -1 on a bad argument */
long cheb_stats_size(const cheb_stats *h, int which);
/* out[f][0..8], DEVICE; center_dev: nfields DEVICE values c_f, or NULL for 0.
 *   0, 1   min and max over the values that are not NaN, with the bits of the element found; +-Inf count as values, -0.0 and
 *          +0.0 compare equal
 *   2, 3   the flat index inside the field of the first element that attains min / max, as a double
 *   4      the number of NaN values.  All NaN: min = +Inf, max = -Inf, both indices -1
 *   5..8   M_p = sum_i W_i (u_i - c_f)^p, p = 1..4, the power by repeated multiplication.  A NaN or Inf propagates into M_p. */
int  cheb_stats_summary(cheb_stats *h, const double *u_dev, const double *center_dev, double *out_dev, void *stream);
/* out[f][2][nbins + 3], DEVICE; slot 0 underflow, 1..nbins the bins, nbins + 1 overflow, nbins + 2 NaN.  Row 0: the mass
 * sum_{i in slot} W_i, or sum W_i c_i with cond_dev (a second set of fields in the same layout; NULL: none): the numerator of a
 * conditional mean.  Row 1: the number of values in the slot.  An empty slot has mass +0.0.  1 <= nbins <= max_bins.
 *   CHEB_STATS_UNIFORM  spec_dev = (lo_f, hi_f) per field, DEVICE (e.g. slots 0, 1 of a summary).  inv = nbins / (hi - lo), one
 *                       IEEE division; u < lo: underflow; t = (u - lo) * inv, one subtraction and one multiplication; t >= nbins
 *                       (or a t that is NaN because hi - lo overflowed): overflow; otherwise bin floor(t).  hi <= lo or a bound
 *                       that is not finite sends every value that is not NaN to overflow.
 *   CHEB_STATS_EDGES    spec_dev = nbins + 1 non-decreasing edges per field, DEVICE.  u < e_0: underflow; u >= e_nbins: overflow;
 *                       otherwise the last b with e_b <= u (so that u < e_{b+1}), found by comparisons only.
 * A NaN value goes to the NaN slot in both modes. */
int  cheb_stats_histogram(cheb_stats *h, const double *u_dev, const double *cond_dev, int mode, int nbins, const double *spec_dev,
                          double *out_dev, void *stream);
/* vel_dev: d fields, whatever nfields is; scale_host: d finite HOST values s_k = 2 / L_k as in cheb_grad_create, or
 * NULL for ones.  out[0] = max_i sum_k |vel_k(i)| r_k[i_k], k ascending, r_k = cheb_stats_rate_host(dims[k], s_k); out[1] = the
 * first flat index that attains it.  A NaN in any component at any node makes out[0] NaN and out[1] the first such node.
 * The handle keeps r of the last scale on the device: a call with another scale forms r again and copies it (sum of dims values,
 * from pageable memory, which the runtime stages before the call returns) ahead of the kernel on `stream`; a call with the same
 * scale copies nothing and relies on the one-stream-at-a-time rule above for its order after that copy. */
int  cheb_stats_cfl(cheb_stats *h, const double *vel_dev, const double *scale_host, double *out_dev, void *stream);

/* ------------------------------------------------------------------------- */
/* Vector calculus of full-grid fields (no counterpart in the reference,      */
/* whose operators differentiate inside their callbacks only).  Fields use    */
/* the full-grid, field-major layout of cheb_modal_*: field f of an array at  */
/* f * N, N = prod(dims), row-major over all nodes.  A VECTOR field is d      */
/* consecutive fields u[v][c], component c along grid direction c.  With      */
/* d_k = the derivative along direction k and s_k = scale[k] (2 / L_k for a   */
/* box of length L_k; default 1):                                             */
/*   grad       out[f*d + k] = s_k d_k s[f]                                   */
/*   tensor     G[v][c][k]   = s_k d_k u[v][c]       (grad of the nv*d fields)*/
/*   div        out[v] = ((s_0 d_0 u[v][0]) + s_1 d_1 u[v][1]) + ...          */
/*   curl       d = 3: w_0 = d_1 u_2 - d_2 u_1, w_1 = d_2 u_0 - d_0 u_2,      */
/*              w_2 = d_0 u_1 - d_1 u_0 (scales included, index = direction); */
/*              d = 2: the one field d_0 u_1 - d_1 u_0; other d: ERR_ARG      */
/*   strain     per vector the d(d+1)/2 fields (0,0), (0,1), .., (d-1,d-1):   */
/*              S_cc = s_c d_c u_c,  S_ck = 1/2 s_k d_k u_c + 1/2 s_c d_c u_k */
/*   laplacian  out[f] = sum_k s_k^2 d_k^2 s[f], k ascending: one sweep with  */
/*              D D (long double, rounded once) for 3 <= n_k <= 256, two D    */
/*              sweeps through `work` for n_k > 256, nothing for n_k = 2      */
/*              (D D = 0 there)                                               */
/* Every output is a list of signed derivative sweeps: the first term is      */
/* stored, the later ones are added to the same array in the order written    */
/* above, the factor of a term (sign, 1/2, scale) multiplies the sweep's      */
/* result.  Results repeat bit for bit.  An output of T terms is within       */
/* (max n + 8 + T) 2^-53 sum_t B_t of the exact value, B_t = |factor| times   */
/* the componentwise weight |D| |u| of the term's sweep.                      */
/* Pointwise invariants of a tensor G[v][c][k] (any array of that layout),    */
/* per vector the selected fields in the order of the bits:                   */
/*   CHEB_INV_DIV      sum_c G_cc                                             */
/*   CHEB_INV_VORT2    sum_{c<k} (G_kc - G_ck)^2      (|curl u|^2 for d = 2,3)*/
/*   CHEB_INV_STRAIN2  S:S = sum_c G_cc^2 + 1/2 sum_{c<k} (G_ck + G_kc)^2     */
/*   CHEB_INV_GAMMA    1/2 S:S: the second invariant of stokes.C:711-717      */
/*   CHEB_INV_Q        1/4 VORT2 - 1/2 STRAIN2                                */
/*   CHEB_INV_NORM2    sum_{c,k} G_ck^2                                       */
/* summed in the index order written (pairs c < k row by row; NORM2 row-major */
/* for d <= 3, and for d > 3 per c: G_cc^2, then G_ck^2, G_kc^2 for k > c).   */
/* A field of T squared (or, DIV, plain) terms is within (T + 4) 2^-53 A of   */
/* the formula evaluated exactly on G, A = the formula with every term taken  */
/* non-negative.  A NaN or Inf at a node stays in that node's outputs.        */
/* ------------------------------------------------------------------------- */
typedef struct cheb_grad cheb_grad;
enum { CHEB_INV_DIV = 1, CHEB_INV_VORT2 = 2, CHEB_INV_STRAIN2 = 4, CHEB_INV_GAMMA = 8, CHEB_INV_Q = 16, CHEB_INV_NORM2 = 32 };

/* 1 <= d <= 10; 2 <= dims[k] <= 1024; fewer than 2^31 nodes; scale: d finite HOST values or NULL (all 1).  The handle owns the
 * differentiation matrices and no work arrays: the calls below allocate nothing on the device and do not synchronise the host. */
int  cheb_grad_create(int d, const int *dims, const double *scale, cheb_grad **out);
int  cheb_grad_destroy(cheb_grad *h);
long cheb_grad_size(const cheb_grad *h);                  /* N = prod(dims); -1: NULL */
long cheb_grad_work_size(const cheb_grad *h, int nfields); /* doubles cheb_grad_laplacian's `work` must hold (0: it may be NULL); -1 on a bad argument */
/* All arrays are DEVICE pointers.  A call takes at most 16 input fields (nfields, or nvec * d) and fewer than 2^31 values per
 * array; no input may overlap an output or the work array (CHEBHIP_ERR_ARG).  Asynchronous on `stream`. */
int  cheb_grad_grad(cheb_grad *h, int nfields, const double *s_dev, double *out_dev, void *stream);
int  cheb_grad_tensor(cheb_grad *h, int nvec, const double *u_dev, double *G_dev, void *stream);
int  cheb_grad_div(cheb_grad *h, int nvec, const double *u_dev, double *out_dev, void *stream);
int  cheb_grad_curl(cheb_grad *h, int nvec, const double *u_dev, double *out_dev, void *stream);
int  cheb_grad_strain(cheb_grad *h, int nvec, const double *u_dev, double *out_dev, void *stream);
int  cheb_grad_laplacian(cheb_grad *h, int nfields, const double *s_dev, double *work_dev, double *out_dev, void *stream);
/* mask: a nonempty set of CHEB_INV_* bits; out: nvec * popcount(mask) fields; 1 <= nvec <= 16.  One kernel launch. */
int  cheb_grad_invariants(cheb_grad *h, int nvec, const double *G_dev, unsigned mask, double *out_dev, void *stream);

/* ------------------------------------------------------------------------- */
/* Between the operators' vectors and full-grid fields.  ell_op and stokes_op */
/* take the reference's vectors: interior nodes only, node-major, the         */
/* components of a node interleaved, and the Dirichlet values in a compact    */
/* array of the boundary nodes in BlockIt (row-major) order (the layout of    */
/* ell_op_set_dirichlet / stokes_op_set_dirichlet).  With m = the number of a */
/* node among the interior nodes and b = its number among the boundary nodes, */
/* both row-major, and l its row-major number among all N nodes:              */
/*   unpack  out[c*N + l] = xi[m*si + oi + c]   (interior node)               */
/*           out[c*N + l] = xb[b*sb + ob + c]   (boundary node)               */
/*   pack    the inverse                                                      */
/* for c < ncomp.  A Stokes state has si = d + 1: velocity oi = 0, ncomp = d  */
/* with sb = d, ob = 0; pressure oi = d, ncomp = 1 with no boundary source.   */
/* A NULL source of unpack gives 0 at its nodes: for a pressure these zeros   */
/* are a placeholder, NOT an extrapolation of the pressure to the boundary.   */
/* A NULL target of pack is skipped; entries of a target that no (node,       */
/* component) addresses -- the other interleaved components -- keep their     */
/* bits.  Values are moved, never computed: every bit arrives.                */
/* ------------------------------------------------------------------------- */
typedef struct cheb_layout cheb_layout;
/* 1 <= d <= 10; 3 <= dims[k] <= 1024; fewer than 2^31 nodes.  The handle owns one int per node on the device. */
int  cheb_layout_create(int d, const int *dims, cheb_layout **out);
int  cheb_layout_destroy(cheb_layout *h);
long cheb_layout_size(const cheb_layout *h, int which);   /* 0: nodes N, 1: interior nodes I, 2: boundary nodes N - I; -1 on a bad argument */
/* The handle's table on the HOST, N ints: map[l] >= 0 is m, map[l] < 0 is -1 - b.  Needs no device. */
int  cheb_layout_map_host(int d, const int *dims, int *map);
/* xi: I * si doubles, xb: (N - I) * sb doubles, out / fields: ncomp * N doubles, all on the DEVICE; 1 <= ncomp, 0 <= oi, oi + ncomp <= si
 * and 0 <= ob, ob + ncomp <= sb for the arrays that are given; the field side must not overlap the vector side.  Asynchronous. */
int  cheb_layout_unpack(cheb_layout *h, int ncomp, const double *xi_dev, long si, long oi, const double *xb_dev, long sb, long ob,
                        double *out_dev, void *stream);
int  cheb_layout_pack(cheb_layout *h, int ncomp, const double *fields_dev, double *xi_dev, long si, long oi, double *xb_dev, long sb, long ob,
                      void *stream);

/* ------------------------------------------------------------------------- */
/* Operator level: the scalar elliptic MatShell (elliptic.C:78-86,250-293).   */
/* Vectors at this boundary are the reference's GLOBAL vectors: interior      */
/* nodes only, row-major (SetupBC, elliptic.C:372-434).  All work vectors     */
/* (w[2+d], gradu[d], eta, deta) live in HBM inside the handle.               */
/* ------------------------------------------------------------------------- */
typedef struct ell_op ell_op;

/* Replaces MatCreate_Elliptic (elliptic.C:250-293) with the homogeneous
 * Dirichlet boundary function DirichletBdy (:468-476); 1 <= d <= 10 as the
 * driver allows (elliptic.C:137).  State after create: eta = 1, deta = 0
 * (elliptic.C:265-266), gradu = 0, dirichlet values = 0. */
int ell_op_create(int d, const int *dims, ell_op **out);
int ell_op_destroy(ell_op *op);                       /* MatDestroy_Elliptic, elliptic.C:343-368 */

long ell_op_local_size(const ell_op *op);             /* N  = prod dims                 */
long ell_op_global_size(const ell_op *op);            /* g  = prod (dims-2): MatShell n */
long ell_op_dirichlet_size(const ell_op *op);         /* N - g                          */

/* Replaces MatMult_Elliptic (elliptic.C:297-339): V = A(eta,deta,gradu) U. */
int ell_op_mult(ell_op *op, const double *U_dev, double *V_dev, void *stream);
int ell_op_mult_host(ell_op *op, const double *U_host, double *V_host);

/* Replaces FormFunction (elliptic.C:481-533): rhs = F(U) - b, and refreshes the
 * operator state eta, deta, gradu used by later ell_op_mult calls.  b may be
 * NULL (treated as 0). */
int ell_op_function(ell_op *op, double gamma, double exponent, const double *U_dev,
                    const double *b_dev, double *rhs_dev, void *stream);
int ell_op_function_host(ell_op *op, double gamma, double exponent, const double *U_host,
                         const double *b_host, double *rhs_host);

/* Sets c->dirichlet (elliptic.C:462,667-668): compact boundary values in
 * BlockIt (row-major) order, ell_op_dirichlet_size() doubles, HOST pointer. */
int ell_op_set_dirichlet(ell_op *op, const double *values_host);

/* Copies operator state to the host for inspection: which = 0 eta, 1 deta,
 * 2+k gradu[k] (each N doubles). */
int ell_op_get_state(ell_op *op, int which, double *dst_host);
/* Overwrites operator state from the host (same `which` codes). */
int ell_op_set_state(ell_op *op, int which, const double *src_host);

/* Slab mode for the multi-GPU path (no counterpart in the serial reference): the handle owns the planes
 * [lo, hi) of grid dimension 0 and its vectors are the serial ones restricted to the slab (contiguous pieces).
 * Sweeps along dimension 0 are delegated: dim0(ctx, 0, 1, in, NULL, alpha, out, stream) must produce
 * out = alpha * D_0 in for one slab field (transpose -> ell_op_pencil_sweep on (dims[0], ncol) -> transpose).
 * ell_op_mult / ell_op_function / set_* / get_state work unchanged on the slab, for any coefficient state. */
typedef int (*ell_dim0_fn)(void *ctx, int kind, int nfields, const double *in_dev, const double *acc_dev,
                           double alpha, double *out_dev, void *stream);
int ell_op_create_slab(int d, const int *dims, int lo, int hi, ell_dim0_fn dim0, void *dim0_ctx, ell_op **out);
int ell_op_pencil_sweep(ell_op *op, long ncol, const double *in_dev, double *out_dev, void *stream);

/* ------------------------------------------------------------------------- */
/* Operator level: the Stokes MatShells (StokesCtx stokes.C:40-65,             */
/* StokesCreate :257-344) with -boundary 0: every boundary node is a velocity  */
/* Dirichlet node, numMixed == 0 (the StokesMixed* hooks are no-ops).          */
/* Vector layouts (StokesSetupDomain, stokes.C:773-938), I = interior nodes:   */
/*   full global  g  = (d+1)*I : [v_0 .. v_{d-1}, p] per interior node         */
/*   velocity     gv = d*I     : node-major        pressure gp = I             */
/*   dirichlet    dv = d*(N-I) : boundary nodes in BlockIt order, node-major   */
/* d = 2 or 3 (StokesPressureReduceOrder, stokes.C:1036).                      */
/* ------------------------------------------------------------------------- */
typedef struct stokes_op stokes_op;

int stokes_op_create(int d, const int *dims, stokes_op **out);      /* StokesCreate, stokes.C:257-344 */
int stokes_op_destroy(stokes_op *op);                               /* StokesDestroy, stokes.C:348-388 */
/* which: 0 local nodes N, 1 interior nodes I, 2 gv, 3 gp, 4 g, 5 dv */
long stokes_op_size(const stokes_op *op, int which);

/* options->rheology (stokes.C:1920-1944): kind 0 = StokesRheologyLinear, 1 = StokesRheologyPower
 * with -hardness, -exponent, -eps, -gamma0 (stokes.C:412-415). */
int stokes_op_set_rheology(stokes_op *op, int kind, double hardness, double exponent,
                           double regularization, double gamma0);
int stokes_op_set_dirichlet(stokes_op *op, const double *values_host);   /* c->dirichlet, dv doubles */
int stokes_op_set_force(stokes_op *op, const double *force_host);        /* c->force, g doubles     */

/* StokesMatMult (stokes.C:499-519) on full global vectors. */
int stokes_op_mult(stokes_op *op, const double *xG_dev, double *yG_dev, void *stream);
/* StokesMatMultVV (:623-676), StokesMatMultPV (:557-566), StokesMatMultVP (:599-619): the inner
 * MatShells MatVV / MatPV / MatVP that the Schur complement (:523-535) and the block
 * preconditioners (:1714-1817) call. */
int stokes_op_mult_vv(stokes_op *op, const double *vG_dev, double *vG_out_dev, void *stream);
int stokes_op_mult_pv(stokes_op *op, const double *vG_dev, double *pG_out_dev, void *stream);
int stokes_op_mult_vp(stokes_op *op, const double *pG_dev, double *vG_out_dev, void *stream);
/* StokesMatMultSchur (:523-535): out = -PV * solve(VV, VP * pG), all on device vectors.
 * `inner_solve(ctx, rhs_dev, sol_dev, stream)` stands for KSPSolve(KSPSchurVelocity) (:531; operators
 * MatVV / MatVVPC, options prefix svel_, :338-341): the PETSc adapter passes a wrapper around that KSP.
 * NULL selects the built-in solver: unpreconditioned restarted GMRES on MatVV with KSP's defaults
 * (restart 30, rtol 1e-5, atol 1e-50, max_it 10000, zero initial guess), see chebhip_fgmres_* below. */
int stokes_op_mult_schur(stokes_op *op, const double *pG_dev, double *pG_out_dev,
                         chebhip_apply_fn inner_solve, void *inner_ctx, void *stream);
/* The same four applies on COMPONENT-MAJOR velocity vectors (component c of interior node n at c * I + n instead of the
 * reference's n * d + c): the layout the block preconditioners keep for their inner Krylov solves (stokes_saddle_*), in which a
 * velocity vector is d stacked scalar fields for MatVVPC's line transforms too -- no (de)interleaving pass per inner iteration.
 * No counterpart in the reference (its vectors are node-major throughout, stokes.C:284-290); pressure vectors are unaffected.
 * stokes_op_mult_schur_cm requires inner_solve, which receives and returns component-major vectors. */
int stokes_op_mult_vv_cm(stokes_op *op, const double *v_cm_dev, double *v_cm_out_dev, void *stream);
int stokes_op_mult_pv_cm(stokes_op *op, const double *v_cm_dev, double *pG_out_dev, void *stream);
int stokes_op_mult_vp_cm(stokes_op *op, const double *pG_dev, double *v_cm_out_dev, void *stream);
int stokes_op_mult_schur_cm(stokes_op *op, const double *pG_dev, double *pG_out_dev,
                            chebhip_apply_fn inner_solve_cm, void *inner_ctx, void *stream);
int stokes_op_set_inner_solver(stokes_op *op, int restart, double rtol, double atol, int max_it);
int stokes_op_inner_iterations(const stokes_op *op);   /* MatVV applies of the last built-in inner solve */
/* Slab mode: the built-in inner solve runs on distributed velocity vectors (see chebhip_fgmres_set_reduce). */
int stokes_op_set_inner_reduce(stokes_op *op, chebhip_reduce_fn reduce, void *ctx);
/* StokesFunction (:680-758): yG = F(xG) - force; refreshes eta, deta, strain. */
int stokes_op_function(stokes_op *op, const double *xG_dev, double *yG_dev, void *stream);
/* Operator state to/from the host: which = 0 eta (N), 1 deta (N), 2+j strain[j] (N*d).  The strain is the symmetrised
 * velocity gradient (stokes.C:718-722): strain[j][k] == strain[k][j]; the Jacobian apply reads the entries with j <= k. */
int stokes_op_get_state(stokes_op *op, int which, double *dst_host);
int stokes_op_set_state(stokes_op *op, int which, const double *src_host);

/* Slab mode for the multi-GPU path (no counterpart in the serial reference).  The handle owns the
 * planes [lo, hi) of grid dimension 0; its vectors are the serial ones restricted to the slab (contiguous
 * pieces, dimension 0 being outermost).  Everything along dimension 0 is delegated to `dim0`:
 *   kind 0: out = (acc ? acc : 0) + alpha * D_0 in   for nfields stacked slab fields of N nodes each
 *   kind 1: out = D_0 (x-line pressure extrapolation of in)              (one field; stokes.C:1064-1074, :611)
 *   kind 2: the first nfields - 1 fields as kind 0 (acc NULL, alpha 1), the LAST field as kind 1: the velocity gradient and the
 *           pressure gradient of a StokesMatMult / StokesFunction along dimension 0 in ONE round trip (the fields are stacked:
 *           the handle keeps the pressure behind the velocity, and the pressure gradient behind the velocity gradient)
 * The driver (spectral-petsc_amd/dist.py) implements it as transpose -> pencil call below -> transpose.
 * All other entry points (mult, mult_vv/pv/vp, function, set_*, get/set_state) work unchanged on the slab. */
typedef int (*stokes_dim0_fn)(void *ctx, int kind, int nfields, const double *in_dev, const double *acc_dev,
                              double alpha, double *out_dev, void *stream);
int stokes_op_create_slab(int d, const int *dims, int lo, int hi, stokes_dim0_fn dim0, void *dim0_ctx, stokes_op **out);
/* Pencil side: arrays (nfields, dims[0], ncol), lines along dimension 0 with stride ncol. */
int stokes_op_pencil_sweep(stokes_op *op, int nfields, long ncol, const double *in_dev, double *out_dev, void *stream);
int stokes_op_pencil_pressure(stokes_op *op, long ncol, double *p_pencil_dev, double *gp0_pencil_dev, void *stream);
/* Kind 2 on the pencils in ONE launch: nvel stacked velocity fields swept with D and, behind them, the pressure field treated as
 * stokes_op_pencil_pressure treats it (two jobs of one launch where the kernels allow it, otherwise the two calls above). */
int stokes_op_pencil_sweep_pressure(stokes_op *op, int nvel, long ncol, double *in_dev, double *out_dev, void *stream);

/* ------------------------------------------------------------------------- */
/* Multi-GPU host for BASELINE config 3: the linear 3-D Poisson    */
/* matvec slab-partitioned along dimension 0, one rank per GPU, two            */
/* all-to-all exchanges per matvec (slab <-> pencil), local sweeps overlapped   */
/* with them on a second stream, accumulation in the serial order k = 0,1,2.   */
/* No counterpart in the serial reference (elliptic.C:262, nk.c:63); any G      */
/* reproduces the G = 1 vector.  Vectors: this rank's contiguous piece of the   */
/* reference's global vector ([chebhip_dist_slab_offset, + local_size)).        */
/* ------------------------------------------------------------------------- */
typedef struct chebhip_dist chebhip_dist;
/* Moves one exchange: send_dev holds, peer-major and contiguous, send_counts[s] doubles for every rank s; the
 * counts received from rank s are recv_counts[s], stored peer-major in recv_dev; ordered on `stream`. */
typedef int (*chebhip_exchange_fn)(void *ctx, const double *send_dev, const long *send_counts, double *recv_dev,
                                   const long *recv_counts, void *stream);
int chebhip_dist_create(int d, const int *dims, int nranks, int rank, chebhip_dist **out);
int chebhip_dist_destroy(chebhip_dist *D);
long chebhip_dist_local_size(const chebhip_dist *D);
long chebhip_dist_slab_offset(const chebhip_dist *D);
/* Transport: grouped ncclSend / ncclRecv on `nccl_comm` (an ncclComm_t of nranks ranks, rank order as at create;
 * rccl.h:700,722,923) -- RCCL is looked up at run time, never linked -- or any other exchange function. */
int chebhip_dist_use_rccl(chebhip_dist *D, void *nccl_comm);
int chebhip_dist_set_exchange(chebhip_dist *D, chebhip_exchange_fn fn, void *ctx);
/* MatMult_Elliptic (elliptic.C:297-339, eta = 1, deta = 0) on the slab: V = -(L_0 + L_1 + ..) U. */
int chebhip_dist_mult(chebhip_dist *D, const double *U_slab_dev, double *V_slab_dev, void *stream);
/* The same matvec on nrhs vectors at once (1..64; U, V: nrhs consecutive slab vectors of chebhip_dist_local_size doubles each): one
 * launch per direction on the stacked slabs / pencils, one pack, ONE grouped exchange each way carrying every vector's blocks, one
 * final sum -- the fixed cost of a launch of 256-point lines and of an RCCL launch is paid per batch, not per vector.  Each vector's
 * result is chebhip_dist_mult's.  For the independent vectors of a block / s-step Krylov method or several right-hand sides; needs a
 * chebhip_comm transport (chebhip_dist_use_comm / _use_rccl).  Collective.  The serial reference has no counterpart. */
int chebhip_dist_mult_batch(chebhip_dist *D, int nrhs, const double *U_slabs_dev, double *V_slabs_dev, void *stream);
/* For hosts without a communicator of their own: rank 0 makes the 128-byte id, the host hands it to every rank. */
int chebhip_rccl_unique_id(void *id128);
int chebhip_rccl_comm_create(int nranks, int rank, const void *id128, void **nccl_comm_out);
int chebhip_rccl_comm_destroy(void *nccl_comm);
/* A chebhip_reduce_fn (ctx = the ncclComm_t): ncclAllReduce of the few doubles a Krylov iteration needs. */
int chebhip_rccl_reduce(void *nccl_comm, double *vals_dev, int count, void *stream);

/* ------------------------------------------------------------------------- */
/* Transports of the slab-partitioned operators.  A chebhip_comm   */
/* carries the exchanges (slab <-> pencil transposes) and the few-double       */
/* reductions of a Krylov iteration among G ranks:                             */
/*   _create_rccl      one process per GPU; each exchange is one grouped       */
/*                     ncclSend/ncclRecv launch over xGMI (rccl.h:700,722,923) */
/*   _create_local     ranks are host threads of ONE process, one stream (and, */
/*                     on a multi-GPU node, one device) each, peer access      */
/*                     between the devices.  A DIRECT transport: the slab      */
/*                     drivers read the peers' arrays in place (no pack, no    */
/*                     messages; two thread rendezvous per round trip), other  */
/*                     exchanges are event-ordered device copies.  Every rank  */
/*                     must make the same sequence of collective calls from    */
/*                     its own thread -- INCLUDING the destroy of a driver     */
/*                     that has run on it (chebhip_dist_destroy,               */
/*                     chebhip_dist_stokes_destroy, chebhip_dist_ell_destroy:  */
/*                     nothing is freed while a peer may still read it).       */
/*   _create_callback  any other transport (the gloo staging of the tests)     */
/*   _create_ipc       ranks are PROCESSES of one node (a launcher's one       */
/*                     process per GPU): the direct route of _create_local     */
/*                     across address spaces -- pointers travel as             */
/*                     (hipIpcMemHandle_t, offset) through a shared-memory     */
/*                     segment, "my arrays are complete" as sequence numbers   */
/*                     in it (hipStreamWriteValue64, one polling launch),      */
/*                     layered over a message transport (_create_rccl, a       */
/*                     callback) that carries the segment exchanges and the    */
/*                     reductions.  The same collective rules as _create_local */
/*                     (destroys included).  Vectors handed to a driver on it  */
/*                     must come from hipMalloc (a caching allocator's blocks  */
/*                     qualify, a virtual-memory allocator's do not).          */
/* ------------------------------------------------------------------------- */
typedef struct chebhip_comm chebhip_comm;
typedef struct chebhip_local_group chebhip_local_group;
typedef struct chebhip_ipc_group chebhip_ipc_group;
/* One exchange: segment i sends send_counts[i] doubles at send_dev[i] to peers[i] and receives recv_counts[i] doubles
 * from it into recv_dev[i]; the k-th segment a rank addresses to peer s meets the k-th segment s addresses to that
 * rank.  The rank's own segments are not passed (device copies inside the library).  Ordered on `stream`. */
typedef int (*chebhip_exchangev_fn)(void *ctx, int nseg, const int *peers, const double *const *send_dev, const long *send_counts,
                                    double *const *recv_dev, const long *recv_counts, void *stream);
int chebhip_comm_create_rccl(void *nccl_comm, int nranks, int rank, chebhip_comm **out);      /* the ncclComm_t is not owned */
int chebhip_local_group_create(int nranks, chebhip_local_group **out);
int chebhip_local_group_destroy(chebhip_local_group *g);   /* after every rank thread has finished; the group outlives its communicators */
int chebhip_local_group_abort(chebhip_local_group *g);   /* a failing rank releases the ranks waiting for it: their calls return an error */
int chebhip_comm_create_local(chebhip_local_group *g, int rank, chebhip_comm **out);          /* call with the rank's device current */
int chebhip_comm_create_callback(int nranks, int rank, chebhip_exchangev_fn xfn, chebhip_reduce_fn rfn, void *ctx, chebhip_comm **out);
/* No wire: every "peer" is the rank itself (the kernels of the direct route with every byte read locally).  For timing the compute
 * side of one rank of an N-rank partition on one GPU; results are meaningless for N > 1. */
int chebhip_comm_create_null(int nranks, int rank, chebhip_comm **out);
/* ... with arrays of their own standing for the peers' k-th posted array (arrays[r], r = 0 .. nranks-1; NULL entries and arrays == NULL:
 * the rank's own): the kernels then read and write nranks distinct arrays, as among real ranks, instead of finding the "peers'" rows
 * in the caches because they are the rank's own.  Each array as large as what the driver posts at index k (chebhip_dist_mult: 0 = the
 * slab vector(s), 1 = the result array of the same size).  Not owned. */
int chebhip_comm_null_set_shadow(chebhip_comm *c, int k, const double *const *arrays);
/* Process ranks.  _open is collective: `name` is a POSIX shared-memory name ("/chebhip-<unique per group>") that rank 0 creates
 * and unlinks again once every rank holds the mapping; call it with the rank's device current.  `inner` (not owned, may be NULL
 * for one rank): a communicator of the same ranks on a message transport.  _close after the communicators and drivers made on
 * the group are gone; _abort releases ranks waiting in a rendezvous (their calls fail). */
int chebhip_ipc_group_open(const char *name, int nranks, int rank, chebhip_ipc_group **out);
int chebhip_ipc_group_close(chebhip_ipc_group *g);
int chebhip_ipc_group_abort(chebhip_ipc_group *g);
int chebhip_comm_create_ipc(chebhip_ipc_group *g, chebhip_comm *inner, chebhip_comm **out);
int chebhip_comm_destroy(chebhip_comm *c);
int chebhip_comm_size(const chebhip_comm *c);
int chebhip_comm_rank(const chebhip_comm *c);
/* A chebhip_reduce_fn (ctx = the chebhip_comm): sums `count` device doubles over the ranks in place; every rank gets the
 * same bits.  For chebhip_fgmres_set_reduce / stokes_op_set_inner_reduce. */
int chebhip_comm_reduce(void *comm, double *vals_dev, int count, void *stream);
/* The linear Poisson host above on any transport (chebhip_dist_use_rccl = _create_rccl + this). */
int chebhip_dist_use_comm(chebhip_dist *D, chebhip_comm *comm);

/* ------------------------------------------------------------------------- */
/* Multi-GPU hosts for BASELINE config 5 and for the elliptic operator in any  */
/* coefficient state, C++ behind this ABI (csrc/slabx.hip): each   */
/* rank owns a slab-mode handle on its planes of grid dimension 0; whatever    */
/* runs along dimension 0 (DV[0], DP[0], D_0, the x-line pressure              */
/* extrapolation stokes.C:1064-1074) is done on pencils: pack -> one grouped   */
/* exchange of all fields of the call -> pencil launch -> exchange -> unpack   */
/* with the AXPY folded in.  The handle returned by *_op() takes every         */
/* stokes_op_* / ell_op_* entry point; its vectors are this rank's contiguous  */
/* pieces of the serial ones (node ranges from *_ranges: [0],[1] interior      */
/* nodes lo/hi, [2],[3] boundary nodes lo/hi, in the serial BlockIt order).    */
/* Every rank must make the same sequence of calls.  No counterpart in the     */
/* serial reference (stokes.C:121 VecCreateSeq).                               */
/* ------------------------------------------------------------------------- */
typedef struct chebhip_dist_stokes chebhip_dist_stokes;
typedef struct chebhip_fdpc chebhip_fdpc;       /* the finite-difference preconditioner, declared below */
int chebhip_dist_stokes_create(int d, const int *dims, chebhip_comm *comm, chebhip_dist_stokes **out);   /* comm NULL: one rank */
int chebhip_dist_stokes_destroy(chebhip_dist_stokes *D);
stokes_op *chebhip_dist_stokes_op(chebhip_dist_stokes *D);        /* owned by D; StokesMatMultSchur's built-in inner solve all-reduces through comm */
/* The preconditioners on slabs (round 4; SURVEY 8f.1 / 8f.3 over ranks): MatVVPC (stokes.C:1160-1241) / FormJacobian's matrix
 * (elliptic.C:537-590) for the slab's unknowns -- chebhip_fdpc handles in slab mode, owned by the driver, line transforms along
 * dimension 0 on pencils through the driver's communicator.  Pass them to chebhip_fdpc_apply / stokes_saddle_create_slab. */
int chebhip_dist_stokes_pc(chebhip_dist_stokes *D, chebhip_fdpc **out);
int chebhip_dist_stokes_ranges(const chebhip_dist_stokes *D, long *ranges4);
typedef struct chebhip_dist_ell chebhip_dist_ell;
int chebhip_dist_ell_create(int d, const int *dims, chebhip_comm *comm, chebhip_dist_ell **out);
int chebhip_dist_ell_destroy(chebhip_dist_ell *D);
ell_op *chebhip_dist_ell_op(chebhip_dist_ell *D);
int chebhip_dist_ell_pc(chebhip_dist_ell *D, chebhip_fdpc **out);
int chebhip_dist_ell_ranges(const chebhip_dist_ell *D, long *ranges4);

/* ------------------------------------------------------------------------- */
/* Krylov driver on device vectors: the caller of the path.     */
/* KSPSolve with KSPFGMRES around MatMult_Elliptic (elliptic.C:181-185) and    */
/* KSPSchurVelocity inside StokesMatMultSchur (stokes.C:531).  Restarted       */
/* flexible GMRES, right preconditioner M (NULL = none; may change between     */
/* applications), classical Gram-Schmidt, convergence on                       */
/* |r| <= max(rtol |b|, atol) as KSPDefaultConverged.  All vectors stay in     */
/* HBM; the host sees one Hessenberg column per iteration.                     */
/* ------------------------------------------------------------------------- */
typedef struct chebhip_fgmres chebhip_fgmres;
int chebhip_fgmres_create(long n, int restart, chebhip_fgmres **out);
/* Vectors distributed over ranks (n = local entries): inner products are completed by `reduce`. NULL = one rank. */
int chebhip_fgmres_set_reduce(chebhip_fgmres *k, chebhip_reduce_fn reduce, void *ctx);
int chebhip_fgmres_destroy(chebhip_fgmres *k);
int chebhip_fgmres_set_tolerances(chebhip_fgmres *k, double rtol, double atol, int max_it);
/* x_nonzero = 0: zero initial guess (x is overwritten); 1: x_dev holds the initial guess. */
int chebhip_fgmres_solve(chebhip_fgmres *k, chebhip_apply_fn A, void *actx, chebhip_apply_fn M, void *mctx,
                         const double *b_dev, double *x_dev, int x_nonzero, void *stream);
int chebhip_fgmres_iterations(const chebhip_fgmres *k);   /* operator applies of the last solve */
double chebhip_fgmres_residual(const chebhip_fgmres *k);  /* last (recurrence) residual norm */
/* KSPConvergedReason of the last solve: 2 rtol, 3 atol, -3 max_it, -9 NaN/breakdown */
int chebhip_fgmres_reason(const chebhip_fgmres *k);

/* ------------------------------------------------------------------------- */
/* The finite-difference preconditioner of the reference:  */
/* FormJacobian's 2d+1-point matrix P on the collocation nodes                  */
/* (elliptic.C:537-590; handed to PCILU, elliptic.C:184-185) and its per-       */
/* component twin MatVVPC of StokesPCSetUp0 (stokes.C:1160-1241).  The matrix   */
/* lives on the device as coefficient arrays; the approximate solve is a fast   */
/* diagonalisation of its constant-coefficient part (dense line transforms on   */
/* the sweep kernel), used alone or inside `sweeps` inner GMRES steps on P.      */
/* Vectors: the operator's global vectors (scalar: g; Stokes: velocity gv).     */
/* ------------------------------------------------------------------------- */
int ell_pc_create(ell_op *op, chebhip_fdpc **out);          /* MatCreateSeqAIJ(.., 1+2d, ..) + PCILU, elliptic.C:163,184 */
int stokes_pc_create(stokes_op *op, chebhip_fdpc **out);    /* MatVVPC, stokes.C:1160-1241 (-pcvel 0)                    */
int chebhip_fdpc_destroy(chebhip_fdpc *pc);
/* Slab mode (the serial reference has no counterpart): the handle preconditions the unknowns of ONE slab of planes of
 * dimension 0; its approximate solve is z = P_1^-1 (r / eta) by fast diagonalisation (sweeps = 0), whose line transforms along
 * dimension 0 run on pencils: `dim0` (collective over the ranks) moves `nfields` stacked interior fields of the slab at in_dev to
 * pencils, applies chebhip_fdpc_pencil_transform and moves the result back to out_dev.  Made by chebhip_dist_stokes_pc /
 * chebhip_dist_ell_pc (csrc/slabx.hip), which supply the callback; i0_offset = interior planes owned by lower ranks. */
typedef int (*chebhip_fdpc_dim0_fn)(void *ctx, int backward, int nfields, const double *in_dev, double *out_dev, void *stream);
int stokes_pc_create_slab(stokes_op *slab_op, long i0_offset, chebhip_fdpc_dim0_fn dim0, void *ctx, chebhip_fdpc **out);
int ell_pc_create_slab(ell_op *slab_op, long i0_offset, chebhip_fdpc_dim0_fn dim0, void *ctx, chebhip_fdpc **out);
int chebhip_fdpc_pencil_transform(chebhip_fdpc *pc, int backward, int nfields, long ncol, const double *in_dev, double *out_dev, void *stream);
/* FormJacobian / StokesPCSetUp0: (re)assemble P from the operator's current eta, deta (and gradu): call after
 * ell_op_function / stokes_op_function or set_state.  Done implicitly on first use. */
int chebhip_fdpc_update(chebhip_fdpc *pc, void *stream);
int chebhip_fdpc_set_sweeps(chebhip_fdpc *pc, int sweeps);  /* inner GMRES steps on P per apply (default 1; 0: P_1^-1 (r/eta) alone) */
/* y = P x: MatMult on the assembled matrix (tests; the defect correction). */
int chebhip_fdpc_mult(chebhip_fdpc *pc, const double *x_dev, double *y_dev, void *stream);
/* z ~= P^-1 r.  Shape of chebhip_apply_fn with ctx = the handle: pass as the M of chebhip_fgmres_solve. */
int chebhip_fdpc_apply(void *pc, const double *r_dev, double *z_dev, void *stream);
/* The same for a Stokes velocity preconditioner (stokes_pc_create*) on component-major vectors (stokes_op_mult_vv_cm): the fast
 * diagonalisation z = P_1^-1 (r / eta) (sweeps = 0) only. */
int chebhip_fdpc_apply_cm(void *pc, const double *r_cm_dev, double *z_cm_dev, void *stream);
/* The steps of the fast-diagonalisation solve (sweeps = 0), one at a time, for tests: the solve itself is a sequence of these
 * calls.  x, y: nf stacked interior fields (component-major on a Stokes handle), distinct (SCALE alone works in place and takes
 * y == x).  A step takes exactly the route the solve takes for this handle, direction k, these arrays and the current options; a
 * mode the solve does not take there is CHEBHIP_ERR_ARG and nothing runs (ZSOLVE on an odd line, on a line outside 66..128
 * points, on a line whose ends differ or under option "fdm_z_separate"; FORWARD on the direction that divides by eta; ...).
 * Slab handles: CHEBHIP_ERR_ARG.  Order of a solve: FORWARD_OVER_ETA (a handle with an operator; a Stokes handle's node-major
 * apply divides while it pulls the components apart and runs FORWARD) or FORWARD along 0, FORWARD along 1 .. d-2, then along d-1
 * either FORWARD_SCALED, or FORWARD and SCALE, or ZSOLVE (which is also the BACKWARD step of d-1); BACKWARD along the rest, d-1
 * first. */
enum { CHEBHIP_FDPC_STEP_FORWARD = 0, CHEBHIP_FDPC_STEP_FORWARD_OVER_ETA = 1, CHEBHIP_FDPC_STEP_FORWARD_SCALED = 2,
       CHEBHIP_FDPC_STEP_ZSOLVE = 3, CHEBHIP_FDPC_STEP_SCALE = 4, CHEBHIP_FDPC_STEP_BACKWARD = 5 };
int chebhip_fdpc_step(chebhip_fdpc *pc, int k, int mode, const double *x_dev, double *y_dev, void *stream);
/* What runs for that step between the handle's own buffers (the arrays of a solve's inner steps), as CHEBHIP_FDPC_ROUTE_* bits;
 * -1 where chebhip_fdpc_step would refuse.  Launches nothing.
 *   RAW: one launch of the 16-byte kernels in a raw mode        TWO_LAUNCH: centro-symmetric plus centro-antisymmetric part
 *   GENERAL: the general sweep kernel (with TWO_LAUNCH)         FUSED_MUL: the pointwise factor rides on the load / store
 *   ETA_PASS: the separate division by eta runs first           ZSOLVE: k_fdm_zsolve16
 *   SCALE3 / SCALE_GENERAL: which modal scaling pass            DENSE: one dense line product with S^-1 itself (the forward
 *   transform where it cannot be one raw launch) */
enum { CHEBHIP_FDPC_ROUTE_RAW = 1, CHEBHIP_FDPC_ROUTE_TWO_LAUNCH = 2, CHEBHIP_FDPC_ROUTE_GENERAL = 4, CHEBHIP_FDPC_ROUTE_FUSED_MUL = 8,
       CHEBHIP_FDPC_ROUTE_ETA_PASS = 16, CHEBHIP_FDPC_ROUTE_ZSOLVE = 32, CHEBHIP_FDPC_ROUTE_SCALE3 = 64, CHEBHIP_FDPC_ROUTE_SCALE_GENERAL = 128,
       CHEBHIP_FDPC_ROUTE_DENSE = 256 };
int chebhip_fdpc_step_route(chebhip_fdpc *pc, int k, int mode);
/* S, S^-1 and lam of the three-point line operator of the preconditioner for a line of P points, as cheb_helmholtz_line_host
 * gives them for the spectral line: the same layout and mode order.  Needs no device. */
int chebhip_fdpc_line_host(int P, double *S, double *Sinv, double *lam);
/* The spectral kind of the same handle: z = (sigma I + A)^-1 (r / eta), exact in the constant-coefficient part (A as for
 * cheb_helmholtz).  chebhip_fdpc_update refreshes eta only; sweeps must stay 0 and chebhip_fdpc_mult is refused (no stencil).
 * A slab-mode operator is refused. */
int ell_pc_create_spectral(ell_op *op, double sigma, chebhip_fdpc **out);           /* z = (sigma I + A)^-1 (r / eta) */

/* ------------------------------------------------------------------------- */
/* Direct Chebyshev Poisson / Helmholtz solves by fast diagonalisation         */
/* (Haidvogel-Zang; no counterpart in the reference, which solves by Krylov).  */
/* A is the operator ell_op_mult applies at eta == 1: per direction the line   */
/* operator A_1 = -(D D)[1..n-1, 1..n-1] on the interior nodes, zero Dirichlet */
/* values.  A_1 = S diag(lam) S^-1 is computed once per extent in long double  */
/* (nonsymmetric eigensolver, modes split by parity), and (sigma I + A)^-1 is  */
/* 2d batched line transforms with the modal weights                           */
/* 1 / (sigma + lam_i + lam_j + ...) -- the pipeline of the finite-difference  */
/* preconditioner below, with the spectral line operator in place of its       */
/* three-point one.                                                            */
/* ------------------------------------------------------------------------- */
typedef struct cheb_helmholtz cheb_helmholtz;      /* (sigma I + A) u = f on interior nodes, zero Dirichlet, eta == 1 */
/* d 1..10, dims[k] 3..258 points (boundary included), sigma >= 0 and finite, nfields 1..16 stacked interior fields (component-
 * major: several right-hand sides per call).  Errors as ell_pc_create.  The handle owns its matrices and work buffers: solve
 * allocates nothing and does not synchronise the host. */
int  cheb_helmholtz_create(int d, const int *dims, double sigma, int nfields, cheb_helmholtz **out);
int  cheb_helmholtz_solve(cheb_helmholtz *h, const double *f_dev, double *u_dev, void *stream);  /* u == f allowed */
int  cheb_helmholtz_apply(void *h, const double *x_dev, double *y_dev, void *stream);            /* chebhip_apply_fn */
int  cheb_helmholtz_destroy(cheb_helmholtz *h);
long cheb_helmholtz_size(const cheb_helmholtz *h);                                   /* nfields * prod(dims - 2); -1: NULL */
/* S (nodal <- modal), S^-1 and lam of A_1 for a line of P points into HOST buffers (M = P - 2; S, Sinv M x M row-major, lam M);
 * needs no device.  Modes by parity: position p < ceil(M/2) the p-th even mode, M-1-q the q-th odd one, each by ascending lam. */
int  cheb_helmholtz_line_host(int P, double *S, double *Sinv, double *lam);          /* M = P - 2, row-major */
/* The solve's own handle, owned by h (any kind of solver handle): for chebhip_fdpc_step / chebhip_fdpc_step_route only. */
chebhip_fdpc *cheb_helmholtz_fdpc(cheb_helmholtz *h);

/* The same solve with a condition alpha u + beta du/dnu = g on every face: Dirichlet (1, 0), Neumann (0, 1),  */
/* Robin otherwise; du/dnu is the outward normal derivative.  An end whose row eliminates it from the collocation of      */
/* -(D D) turns each line operator into A~ = -(DD)_II - (DD)_IB Q, with u_B = Q u_I + B_BB^-1 g; equal ends keep the      */
/* parity split, different ends one dense decomposition (two-launch transforms).  The unknowns stay the interior nodes:    */
/* (sigma I + sum_k A~_k) u_I = f_I + sum_k L_k g (the lift), then the boundary of the full grid is rebuilt direction by   */
/* direction (k = 0 .. d-1: every node is set once, by the highest direction in which it is an end node, from that face's  */
/* condition).  sigma = 0 with Neumann on every face is singular: the product of the zero modes gets weight 0, so the      */
/* solution has no component along it (w . u_I = 0, w the product of the lines' zero-mode rows of S^-1) and that part of  */
/* the lifted right-hand side is discarded.                                                                               */
/* bc: 4*d doubles, per direction k: alpha_first, beta_first, alpha_last, beta_last
 * ("first" = grid index 0 = x=+1, "last" = index n = x=-1; du/dnu outward).  alpha, beta >= 0, finite, not both 0.  Other
 * limits as cheb_helmholtz_create, and nfields * N <= 2^31 - 1.  cheb_helmholtz_solve / _apply on such a handle solve the
 * interior problem with g = 0 (usable as Fgmres's M). */
int  cheb_helmholtz_create_bc(int d, const int *dims, const double *bc, double sigma, int nfields, cheb_helmholtz **out);
/* f: nfields x G interior values; g: nfields x (N-G) compact boundary values in row-major node order (the
 * ell_op_set_dirichlet layout), NULL = zero data; u: nfields x N full-grid values.  u may not alias f or g.  Asynchronous
 * on the stream, allocates nothing. */
int  cheb_helmholtz_solve_bc(cheb_helmholtz *h, const double *f_dev, const double *g_dev, double *u_dev, void *stream);
long cheb_helmholtz_full_size(const cheb_helmholtz *h);       /* nfields * N       */
long cheb_helmholtz_boundary_size(const cheb_helmholtz *h);   /* nfields * (N - G) */
int  cheb_helmholtz_singular(const cheb_helmholtz *h);        /* 1: the zero mode is dropped */
/* S, Sinv (M x M), lam (M) of A~, Q (2 x M), L (M x 2), B_BB^-1 (2 x 2), row-major HOST buffers, for a line of P points with
 * bc4 = {alpha_first, beta_first, alpha_last, beta_last}.  Equal ends: the parity layout of cheb_helmholtz_line_host (all
 * Dirichlet: its matrices, bit for bit); different ends: modes by ascending lam.  Neumann at both ends: lam = 0 exactly. */
int  cheb_helmholtz_line_bc_host(int P, const double *bc4, double *S, double *Sinv, double *lam,
                                 double *Q /* 2 x M */, double *L /* M x 2 */, double *Binv /* 2 x 2 */);
/* The same solve on a box: scale[k] = s_k = 2 / L_k > 0 and finite (d HOST values; NULL: all 1, the handle of _create_bc with the
 * same bits), (sigma - sum_k s_k^2 d_k^2) u = f with alpha u + beta s_k du/dnu = g on the faces of direction k: beta multiplies
 * the physical outward normal derivative.  The line of direction k is the line of the ends (alpha, beta s_k) with lam and L times
 * s_k^2; directions share a line only if extent, ends and scale agree.  singular as before: sigma = 0 and alpha = 0 on
 * every face.  Solved with cheb_helmholtz_solve / _solve_bc. */
int  cheb_helmholtz_create_box(int d, const int *dims, const double *bc, const double *scale, double sigma, int nfields, cheb_helmholtz **out);
/* cheb_helmholtz_line_bc_host for a direction of scale s (s = 1: its bits) */
int  cheb_helmholtz_line_box_host(int P, const double *bc4, double s, double *S, double *Sinv, double *lam,
                                  double *Q /* 2 x M */, double *L /* M x 2 */, double *Binv /* 2 x 2 */);

/* ------------------------------------------------------------------------- */
/* Projection onto discretely divergence-free fields on a box.   */
/* A velocity is d stacked full-grid fields u[v][k] (the layout of            */
/* cheb_grad_div), s_k = scale[k], d_k the derivative sweep of direction k    */
/* (index 0 is x = +1: the outward normal derivative is +s_k d_k at index 0,  */
/* -s_k d_k at index n_k - 1).  Every face (k, end) is a WALL (the normal     */
/* velocity of the result is prescribed) or OPEN (phi = 0, the normal         */
/* velocity is free).  phi, a full-grid field, solves the collocation problem */
/*   interior nodes:  sum_k s_k^2 (D D)_k phi = sum_k s_k d_k u_k             */
/*   boundary node b, k the HIGHEST direction in which b is an end node:      */
/*     wall:  +- s_k d_k phi = +- u_k - flux_b      open:  phi = 0            */
/* (flux: the prescribed outward normal velocity, compact boundary layout of  */
/* cheb_helmholtz_solve_bc) and the result is  out_k = u_k - s_k d_k phi  at  */
/* every node.  With an open face div(out) = 0 at the interior nodes to       */
/* rounding; with walls only the problem is singular, the solver drops the    */
/* constant-like mode and div(out) equals ONE constant c(u) at the interior   */
/* nodes (the part of the right-hand side along the dropped mode: spectrally  */
/* small for resolved fields, O(1) for noise).  The normal component of out   */
/* equals flux at every wall node for the direction that supplies the node's  */
/* condition; an edge or corner node meets the condition of its highest end   */
/* direction only, its normal components in lower directions are not          */
/* controlled.  P(P u) = P u to rounding; the gradient of a nodal field maps  */
/* to 0 at every node.                                                        */
/* ------------------------------------------------------------------------- */
typedef struct cheb_project cheb_project;
enum { CHEB_FACE_WALL = 0, CHEB_FACE_OPEN = 1 };
/* 1 <= d <= 10; 3 <= dims[k] <= 258; faces: 2 d ints, faces[2 k + end] (end 0 = index 0), NULL = walls everywhere; scale as
 * cheb_helmholtz_create_box; nvec vectors per call, nvec * d <= 16, fewer than 2^31 values per array.  The handle owns a cheb_grad,
 * a box Helmholtz handle (sigma = 0, nvec fields), two node tables and the solver's f and g: apply allocates nothing. */
int  cheb_project_create(int d, const int *dims, const int *faces, const double *scale, int nvec, cheb_project **out);
int  cheb_project_destroy(cheb_project *h);
long cheb_project_size(const cheb_project *h, int which);  /* 0: nodes N, 1: interior nodes G, 2: boundary nodes N - G; -1 on a bad argument */
int  cheb_project_singular(const cheb_project *h);         /* 1: walls everywhere, the constant-like mode is dropped; -1: NULL */
/* face[b] = 2 k + end of the face whose condition boundary node b takes, N - G HOST ints in row-major boundary order.  No device. */
int  cheb_project_faces_host(int d, const int *dims, int *face);
/* DEVICE arrays: u, out nvec * d * N; phi nvec * N (required: the potential comes back in it); flux nvec * (N - G) or NULL (0).
 * out may BE u (in place); any other overlap of two arrays is CHEBHIP_ERR_ARG.  Divergence into phi, one launch for f and g, the
 * direct solve, one accumulating sweep per component of out.  Asynchronous on `stream`; the same input gives the same bits. */
int  cheb_project_apply(cheb_project *h, const double *u_dev, const double *flux_dev, double *phi_dev, double *out_dev, void *stream);

/* ------------------------------------------------------------------------- */
/* Functions of the Helmholtz operator.  B = sigma - sum_k s_k^2  */
/* d_k^2 with the faces of cheb_helmholtz_create_box is diagonal in the        */
/* solver's line eigenvectors S = S_0 x .. x S_{d-1}; one call computes, for   */
/* every output field o,                                                       */
/*   y_o = S [ sum_{terms t with out = o} c_t f_t(s) .* (S^-1 x_{i_t}) ]       */
/* with s = ((sigma + l_0[i_0]) + l_1[i_1]) + ... the eigenvalue sum of a mode */
/* (the association of the solver's weights) and the terms of an output added  */
/* in table order into a sum that starts at 0: the same input gives the same   */
/* bits.  An output without a term is 0.  The kinds, z = -tau s:               */
/*   ONE   1                                                                   */
/*   INV   1 / s               (s == 0: 0, the dropped mode of a singular box) */
/*   RES   1 / (par + tau s)   (a zero denominator: 0)                         */
/*   EXP   e^z                                                                 */
/*   PHI1..PHI3  phi_k(z), phi_0 = e^z, phi_{k+1}(z) = (phi_k(z) - 1/k!) / z   */
/*         (z == 0: 1/k!)                                                      */
/*   POW   s^par               (s == 0: 0, or 1 for par == 0; s < 0: NaN)      */
/* EXP and PHI* need a finite tau >= 0, RES finite par and tau, POW a finite   */
/* par; what a kind does not read is ignored.                                  */
/* ------------------------------------------------------------------------- */
typedef struct cheb_opfun cheb_opfun;
enum { CHEB_OPFUN_ONE = 0, CHEB_OPFUN_INV, CHEB_OPFUN_RES, CHEB_OPFUN_EXP, CHEB_OPFUN_PHI1, CHEB_OPFUN_PHI2, CHEB_OPFUN_PHI3, CHEB_OPFUN_POW };
typedef struct { int out, in, kind; double coef, tau, par; } cheb_opfun_term;
/* d, dims, bc, scale, sigma as cheb_helmholtz_create_box with the same limits, except that bc may be NULL (Dirichlet on every
 * face: the lines of cheb_helmholtz_create; scale then has to be NULL too).  nin input and nout output fields per call, 1..16
 * each: stacked interior fields of G = prod(dims - 2) values.  The handle owns its lines and scratch; a new handle has no term. */
int  cheb_opfun_create(int d, const int *dims, const double *bc, const double *scale, double sigma, int nin, int nout, cheb_opfun **out);
int  cheb_opfun_destroy(cheb_opfun *h);
/* Replaces the term table (0..32 terms, HOST array).  Host work only: no device call, no allocation; the table travels with each
 * apply as a kernel argument, so a call queued earlier keeps the table it was issued with. */
int  cheb_opfun_set_terms(cheb_opfun *h, int nterms, const cheb_opfun_term *terms);
/* set_terms' checks for a handle of nin inputs and nout outputs, without one: 0 or CHEBHIP_ERR_ARG.  Needs no device. */
int  cheb_opfun_check_terms(int nin, int nout, int nterms, const cheb_opfun_term *terms);
/* x: nin * G, y: nout * G DEVICE values.  d forward line transforms of nin fields, one launch of the mixing kernel, d backward
 * line transforms of nout fields.  y may BE x when nin == nout; any other overlap is CHEBHIP_ERR_ARG.  Asynchronous on `stream`,
 * allocates nothing. */
int  cheb_opfun_apply(cheb_opfun *h, const double *x_dev, double *y_dev, void *stream);
/* Handles made with bc: the same, each output written as a full-grid field (nout * N values) whose boundary values are those of
 * the homogeneous conditions, u_B = Q u_I (the extension of cheb_helmholtz_solve_bc with g = NULL).  yfull may not overlap x. */
int  cheb_opfun_apply_full(cheb_opfun *h, const double *x_dev, double *yfull_dev, void *stream);
long cheb_opfun_size(const cheb_opfun *h, int which);      /* 0: nin * G, 1: nout * G, 2: nout * N; -1 on a bad argument */
int  cheb_opfun_singular(const cheb_opfun *h);             /* 1: sigma = 0 and alpha = 0 on every face (a mode with s == 0); -1: NULL */
/* f(s) of one kind for HOST doubles: z and f in long double, rounded once (phi_k by a series without cancellation for
 * |z| <= 1).  Needs no device. */
int  cheb_opfun_weight_host(int kind, double tau, double par, double s, double *w);
int  cheb_opfun_weights_host(int kind, double tau, double par, long n, const double *s, double *w);   /* the same for n HOST values */
/* w[i] = f(s[i]) for n DEVICE values by the mixing kernel's own device functions: the weights of a spectrum. */
int  cheb_opfun_eval(int kind, double tau, double par, const double *s_dev, long n, double *w_dev, void *stream);

/* ------------------------------------------------------------------------- */
/* The block preconditioners of the Stokes saddle-point system:  */
/* StokesPCApply0..3 (stokes.C:1714-1817) with the inner solves KSPVelocity,    */
/* KSPSchur and KSPSchurVelocity (stokes.C:328-341) on device vectors.          */
/* ------------------------------------------------------------------------- */
typedef struct stokes_saddle stokes_saddle;
int stokes_saddle_create(stokes_op *op, stokes_saddle **out);
/* On slabs: slab_op = chebhip_dist_stokes_op(D), slab_pc = chebhip_dist_stokes_pc(D) (borrowed), reduce / reduce_ctx =
 * chebhip_comm_reduce with the driver's communicator.  The inner solves and the removal of the constant pressure mode complete
 * their sums over the ranks; stokes_saddle_apply is then collective.  The serial reference has no counterpart.
 * Destroy order: the saddle BORROWS slab_op, slab_pc and reduce_ctx -- destroy it before chebhip_dist_stokes_destroy(D) (which frees
 * the pc) and before the communicator. */
int stokes_saddle_create_slab(stokes_op *slab_op, chebhip_fdpc *slab_pc, chebhip_reduce_fn reduce, void *reduce_ctx, stokes_saddle **out);
int stokes_saddle_destroy(stokes_saddle *s);
/* -pc_saddle_type (stokes.C:177-187): 0 block LU, 1 upper triangular, 2 block diagonal, 3 lower triangular. */
int stokes_saddle_set_type(stokes_saddle *s, int type);
/* Inner solves: which = 0 KSPVelocity (-vel_), 1 KSPSchur (-schur_), 2 KSPSchurVelocity (-svel_); max_it GMRES
 * iterations at most (restart 30) to relative tolerance rtol.  For the two velocity solves max_it = 0 means
 * -ksp_type preonly: one application of the MatVVPC solve.  Defaults (README:43): 4 / 3 / preonly, rtol 1e-5. */
int stokes_saddle_set_inner(stokes_saddle *s, int which, int max_it, double rtol);
/* KSPSchur's preconditioner: 1 (default) = PCJACOBI with the diagonal of StokesMatGetDiagonalSchur (stokes.C:330-331,
 * :538-553: 1/eta at the interior nodes, so residuals are multiplied by the viscosity; left-preconditioned as PETSc's
 * GMRES is), 0 = none (-schur_pc_type none). */
int stokes_saddle_set_schur_jacobi(stokes_saddle *s, int on);
/* Inner GMRES steps on MatVVPC inside its approximate solve (see chebhip_fdpc_set_sweeps); default 0. */
int stokes_saddle_set_pc_sweeps(stokes_saddle *s, int sweeps);
/* StokesPCSetUp0 (stokes.C:1160-1241): re-assemble MatVVPC from the operator's current eta. */
int stokes_saddle_setup(stokes_saddle *s, void *stream);
/* y = M^-1 x on full global vectors (the pressure part of y has zero mean: KSPSetNullSpace, stokes.C:1017-1019).
 * Shape of chebhip_apply_fn with ctx = the handle. */
int stokes_saddle_apply(void *s, const double *x_dev, double *y_dev, void *stream);
/* MatVV applies (which = 0) / MatSchur applies (1) spent by the inner solves of the last apply. */
int stokes_saddle_iterations(const stokes_saddle *s, int which);

/* ------------------------------------------------------------------------- */
/* Periodic (Fourier) directions.  A periodic direction of n     */
/* points, 2 <= n <= 256, has the nodes x_j = -1 + 2 j / n (period 2, no      */
/* duplicated end point) and runs on the same dense line kernels as a CGL     */
/* line.  basis[k] = 0: CGL (two walls), 1: Fourier.                          */
/* ------------------------------------------------------------------------- */
enum { CHEB_BASIS_CGL = 0, CHEB_BASIS_FOURIER = 1 };
enum { CHEB_FOURIER_COS = 0, CHEB_FOURIER_SIN = 1, CHEB_FOURIER_NYQUIST = 2 };
/* Host-side matrices; they need no device.  Long double, rounded once; n x n row-major.
 *   diff_matrix  order 1: D_F = pi D_theta, D_theta[i][j] = 1/2 (-1)^(i-j) cot(pi (i-j) / n) for even n, 1/2 (-1)^(i-j) /
 *                sin(pi (i-j) / n) for odd n, zero diagonal; order 2: D_F D_F (NOT the textbook second-derivative matrix: for
 *                even n the two differ at the Nyquist vector (-1)^j, which D_F D_F annihilates)
 *   modes        position p of the coefficient layout -> wavenumber k[p] and kind[p] (CHEB_FOURIER_*): the parity layout of
 *                cheb_helmholtz_line_host about the flip j -> n-1-j, which reflects x about c = -1/n.  Even modes at p < ceil(n/2):
 *                the constant (COS, k = 0) at p = 0 and cos(pi k (x - c)) at p = k; odd modes at n-1-q: for even n the Nyquist
 *                vector (k = n/2) at q = 0 and sin(pi k (x - c)) at q = k, for odd n sin at q = k - 1; 1 <= k <= floor((n-1)/2)
 *   modal_matrix which = 1 backward B (column p = mode p with amplitude 1: the constant's coefficient is the mean), 0 forward
 *                T = B^-1; every column of B and every row of T is even or odd under the flip bit for bit
 *   line         -scale^2 D_F D_F = S diag(lam) S^-1 in closed form: S = B, Sinv = T, lam = (pi k scale)^2 and exactly 0 for the
 *                constant and the Nyquist vector */
int  cheb_fourier_nodes_host(int n, double *x);
int  cheb_fourier_diff_matrix_host(int n, int order, double *D);
int  cheb_fourier_modes_host(int n, int *k, int *kind);
int  cheb_fourier_modal_matrix_host(int n, int which, double *M);
int  cheb_fourier_line_host(int n, double scale, double *S, double *Sinv, double *lam);
/* cheb_grad_create with a basis per direction (basis not NULL): a Fourier direction differentiates with D_F, and the Laplacian
 * with D_F D_F, through the same sweeps.  All-zero basis: the handle and the bits of cheb_grad_create. */
int  cheb_grad_create_basis(int d, const int *dims, const double *scale, const int *basis, cheb_grad **out);
/* cheb_modal_create with a basis per direction: forward / backward / filter use T, B and B diag(sigma) T of
 * cheb_fourier_modal_matrix_host on a Fourier direction (sigma per coefficient POSITION), integrate the weight 2 / n. */
int  cheb_modal_create_basis(int d, const int *dims, int nfields, const int *basis, cheb_modal **out);
/* cheb_helmholtz_create_box with a basis per direction.  A Fourier direction k has dims[k] unknowns (2 <= dims[k] <= 256), no faces
 * and no entries in g; its four bc values are not read (bc may be NULL when every direction is periodic).  The unknown-node arrays
 * are row-major over M_k = dims[k] (Fourier) or dims[k] - 2 (wall) points per direction, size = nfields * prod M_k; boundary_size =
 * nfields * (N - G) counts the nodes that are end nodes of some wall direction, in row-major order.  singular: sigma = 0 and every
 * direction periodic or Neumann / Neumann; the solve then drops every product of zero-eigenvalue modes (the constants and, on a
 * periodic direction of even extent, the Nyquist vector).  All-zero basis: cheb_helmholtz_create_box itself. */
int  cheb_helmholtz_create_basis(int d, const int *dims, const int *basis, const double *bc, const double *scale, double sigma, int nfields,
                                 cheb_helmholtz **out);

/* The toolbox on periodic directions.  The interpolant of n periodic values is I u(x) = sum_j u_j r_j(x),
 *   r_j(x) = (1/n) [1 + 2 sum_{k=1}^{K} cos pi k (x - x_j)]                             n odd,  K = floor(n/2)
 *   r_j(x) = (1/n) [1 + 2 sum_{k=1}^{K-1} cos pi k (x - x_j) + cos pi K (x - x_j)]      n even
 * Every _basis call refuses a NULL basis ("basis is NULL") and any value other than CHEB_BASIS_*; an all-zero basis is the old
 * create call itself: the same handle, the same bits. */
/* cheb_dealias_create with a basis per direction.  A Fourier direction of n coarse (2 .. 256) and m >= n fine nodes -1 + 2 i / m uses
 * R[i][j] = r_j(y_i), G = R D_F (long double product, rounded once) and P[i][j] = (1/m) [1 + 2 sum_{k=1}^{K} cos pi k (x_i - y_j)]: the
 * fine-grid function's Fourier series cut at |k| <= K, at the coarse nodes (m == n: the identity).  For even n the wavenumber K is
 * kept with what the coarse grid sees of it: the square of the Nyquist vector (-1)^j, 1 at every node, truncates to 1/2 at every
 * node.  Default fine size 3 floor(n/2) + 1 (NOT ceil(3n/2): the product reaches wavenumber 2K, which must not fold onto |k| <= K);
 * dims_fine[k] up to 1024 as before.  Schedule, buffers and launches are those of cheb_dealias_create. */
int  cheb_dealias_create_basis(int d, const int *dims, const int *dims_fine, const int *basis, int nfields, cheb_dealias **out);
int  cheb_dealias_fine_size_basis(int n, int basis);       /* the default fine size of one direction; -1 on a bad n or basis */
/* cheb_dealias_matrix_host for one direction of the given basis (CHEB_BASIS_CGL: that call itself) */
int  cheb_dealias_matrix_basis_host(int n, int m, int which, int basis, double *A);
/* cheb_project_create with a basis per direction: cheb_grad_create_basis and cheb_helmholtz_create_basis underneath.  A periodic
 * direction has 2 <= dims[k] <= 256 and no faces (its two face codes are not read).  The unknowns are the nodes interior in every
 * WALL direction (cheb_project_size which = 1), the boundary nodes the end nodes of some wall direction (which = 2; the highest such
 * direction names the face), both in the solver's row-major order.  Every direction periodic: no boundary, flux must be NULL.
 * div(out): every direction periodic -- zero to rounding at EVERY node (D_F's range holds neither the constant nor the Nyquist
 * vector, so the right-hand side has no component along a dropped mode); an open face -- zero to rounding at the unknown nodes;
 * walls only in the wall directions (a channel; singular) -- free along the dropped modes' right eigenvectors: constant along the
 * wall directions and, per periodic direction, the constant or, for an EVEN extent, the Nyquist vector (-1)^j.  With odd periodic
 * extents that is one constant, as for all-wall handles; with e even ones 2^e coefficients (small for resolved fields). */
int  cheb_project_create_basis(int d, const int *dims, const int *basis, const int *faces, const double *scale, int nvec, cheb_project **out);
int  cheb_project_faces_basis_host(int d, const int *dims, const int *basis, int *face);    /* cheb_project_faces_host on that geometry */
/* cheb_opfun_create over cheb_helmholtz_create_basis: stacked fields in the solver's unknown layout.  bc may be NULL only when every
 * direction is periodic.  A mode with s == 0 (sigma = 0, every direction periodic or Neumann / Neumann: every product of constants
 * and Nyquist vectors) gets what cheb_opfun_term's kinds give s == 0 on any singular handle.  apply_full works on every such handle;
 * with every direction periodic the unknown layout is the full grid and it equals apply. */
int  cheb_opfun_create_basis(int d, const int *dims, const int *basis, const double *bc, const double *scale, double sigma, int nin, int nout,
                             cheb_opfun **out);
/* cheb_points_create with a basis per direction.  On a periodic direction (2 <= dims[k] <= 256) the rows are those of I u above, in
 * the barycentric form r_j ~ (-1)^j cot(pi (x - x_j) / 2) (n even), (-1)^j / sin(pi (x - x_j) / 2) (n odd), built on the device in
 * the nearest-node form of the CGL rows.  Unlike a CGL direction, which extrapolates outside [-1, 1], ANY finite coordinate is
 * WRAPPED (x - 2 rint(x / 2), exact); a coordinate that is a node modulo the period gives the exact unit row, NaN or +-Inf a row
 * of NaN.  The derivative rows are the derivative of the same function (at a node: the row of D_F).  Every call that takes rows
 * (eval, eval_grid, eval_grad, eval_deriv, spread, spread_deriv) works unchanged; CHEB_SPREAD_DELTA divides by the weight 2 / n of
 * a periodic direction, so that cheb_modal_integrate (same basis) of the spread field against phi is sum_p s_p phi(x_p) for every
 * phi of the grid's trigonometric space. */
int  cheb_points_create_basis(int d, const int *dims, int nfields, const int *basis, cheb_points **out);
/* m rows r_j(x_i) (deriv = 0) or r_j'(x_i) (deriv = 1) of a periodic direction of n nodes into R (m x n, row-major): the cosine
 * sums of I u with x wrapped as above, long double, rounded once; HOST arrays, no device.  NaN or +-Inf: a row of NaN. */
int  cheb_points_fourier_matrix_host(int n, int m, const double *x, int deriv, double *R);

/* ------------------------------------------------------------------------- */
/* The variable-coefficient Helmholtz operator  c(x) u - div(kappa(x) grad u)  */
/* and its solve (no counterpart in the reference, whose only      */
/* variable-coefficient operator is MatMult_Elliptic: one field, zero          */
/* Dirichlet values, the unit cube).  Everything is on the conventions of      */
/* cheb_helmholtz_create_basis: dims, basis, bc, scale, nfields and their      */
/* limits, the unknown layout (interior nodes of a wall direction, all nodes   */
/* of a periodic one, row-major, fields stacked), the compact boundary data g. */
/* ------------------------------------------------------------------------- */
/* For unknowns x and boundary data g (NULL = 0):
 *   1. W = the full-grid extension: on every line of a wall direction k the two end values are Q_k x_line + B_BB^-1 g, the matrices
 *      of cheb_helmholtz_line_box_host for that direction's ends and scale -- the condition alpha u + beta s_k du/dnu = g, WITHOUT
 *      kappa: for Neumann data of the flux kappa du/dnu the caller divides g by kappa at the face (conormal Robin data is not built);
 *   2. y = c x + sum_k (-s_k^2) D_k( kappa D_k W ) at the unknown nodes, D the CGL matrix on a wall direction and D_F on a periodic
 *      one, directions ascending.  Direction k reads face values of direction k only; edge and corner values influence nothing.
 * kappa: one full-grid field (prod dims values, read at face nodes too), finite and > 0, shared by the stacked fields; c: a scalar
 * >= 0 or one full-grid field >= 0.  Results repeat bit for bit; a NaN in one field leaves the others' bits alone. */
typedef struct cheb_varhelm cheb_varhelm;
/* basis NULL: walls everywhere.  Errors as cheb_helmholtz_create_basis.  The handle owns its work memory (cheb_varhelm_work_bytes:
 * its own arrays, the buffers and matrices of the inner direct solve, and the Krylov bases, (2 restart + 1) vectors made by the first
 * solve and kept; a solve with another restart length waits for the stream, frees them and makes its own, so only one set exists). */
int  cheb_varhelm_create(int d, const int *dims, const int *basis, const double *bc, const double *scale, int nfields, cheb_varhelm **out);
int  cheb_varhelm_destroy(cheb_varhelm *h);
long cheb_varhelm_size(const cheb_varhelm *h);            /* nfields * unknowns         */
long cheb_varhelm_full_size(const cheb_varhelm *h);       /* nfields * N                */
long cheb_varhelm_boundary_size(const cheb_varhelm *h);   /* nfields * (N - unknowns)   */
long cheb_varhelm_work_bytes(const cheb_varhelm *h);
/* Copies kappa and c (c_dev NULL: the scalar c_scalar) into the handle; device arrays of prod dims values.  Synchronous: it drains
 * the device first (one checking pass: CHEBHIP_ERR_ARG if kappa is not finite and > 0 or c not finite and >= 0 at some node, and the
 * handle keeps what it had), sets the preconditioner's shift sigma_p = mean of c / kappa over the unknown nodes, and returns when
 * the copies are complete, so a later call on any stream sees the new coefficients. */
int  cheb_varhelm_set_coefficients(cheb_varhelm *h, const double *kappa_dev, const double *c_dev, double c_scalar, void *stream);
double cheb_varhelm_sigma(const cheb_varhelm *h);         /* sigma_p; -1 before set_coefficients */
/* 1: c == 0 and every direction periodic or Neumann / Neumann (the inner direct solve is singular): solve refuses; -1: no coefficients yet */
int  cheb_varhelm_singular(const cheb_varhelm *h);
/* Tensor diffusivity and advection, d = 2 or 3 (any other d: CHEBHIP_ERR_ARG).  With W the extension above and
 * directions ascending in every sum:
 *     G_k = s_k D_k W  (k < d, the whole grid),   F_j = sum_k K_jk G_k,   a = sum_k v_k G_k,   y = c x + a - sum_j s_j D_j F_j
 * at the unknown nodes: c u + v . grad u - div(K grad u).  K_dev: d (d + 1) / 2 full-grid fields one after the other, the
 * diagonal first, then the upper triangle row-major -- d = 3: 00 11 22 01 02 12; d = 2: 00 11 01 -- finite and positive definite
 * at EVERY node (it is read at face nodes too; the test is the leading principal minors in double: K00 > 0, K00 K11 - K01^2 > 0,
 * det K > 0).  vel_dev: d full-grid fields, finite, or NULL (no advection).  c as in set_coefficients.  One K, v and c for all
 * stacked fields.  The faces carry alpha u + beta s_k du/dnu = g with NEITHER K NOR v (conormal data n . K grad u is not built).
 * Unlike the scalar operator this one reads the tangential derivatives of W on the faces, hence the edge values of the extension
 * (every boundary node set once, by the highest direction in which it is an end node); corner values influence nothing.
 * Synchronous like set_coefficients, with the same refusals (the handle keeps what it had); the first call allocates the copies
 * of K and v and d gradient grids per field (cheb_varhelm_work_bytes grows by them).  The preconditioner becomes
 * H(sigma_p)^-1 (r / kbar), kbar = trace(K) / d, sigma_p = mean of c / kbar over the unknown nodes: it ignores v and the
 * anisotropy.  Every other entry point works as in the scalar mode (the null space of a singular handle is the same);
 * cheb_varhelm_set_coefficients puts the handle back into the scalar mode, and after either call it gives the bits of a fresh
 * handle that received that call alone. */
int  cheb_varhelm_set_tensor(cheb_varhelm *h, const double *K_dev, const double *vel_dev, const double *c_dev, double c_scalar, void *stream);
#define CHEB_VARHELM_MODE_NONE   0
#define CHEB_VARHELM_MODE_SCALAR 1
#define CHEB_VARHELM_MODE_TENSOR 2
int  cheb_varhelm_mode(const cheb_varhelm *h);            /* which setter came last; -1: NULL */
/* y = the linear operator (g = 0) of x; out = f - (the operator at g)(x).  Asynchronous on the stream, no allocation; the output
 * may overlap no input (CHEBHIP_ERR_ARG).  cheb_varhelm_apply: mult with the shape of chebhip_apply_fn (ctx = the handle). */
int  cheb_varhelm_mult(cheb_varhelm *h, const double *x_dev, double *y_dev, void *stream);
int  cheb_varhelm_apply(void *h, const double *x_dev, double *y_dev, void *stream);
int  cheb_varhelm_residual(cheb_varhelm *h, const double *x_dev, const double *f_dev, const double *g_dev, double *out_dev, void *stream);
/* z = H(sigma_p)^-1 (r / kappa), H the direct solve cheb_helmholtz_create_basis of the same arguments.  Shape of chebhip_apply_fn;
 * z may be r. */
int  cheb_varhelm_precond(void *h, const double *r_dev, double *z_dev, void *stream);
/* b = residual(0, f, g); chebhip_fgmres (restart, rtol, atol, max_it) on A = mult with the right preconditioner precond, from x = 0
 * (x_nonzero = 0) or from the guess in x_dev; x_dev: the unknowns; u_full_dev (may be NULL): the full grid by the extension of
 * cheb_helmholtz_solve_bc (every boundary node set once, by the highest direction in which it is an end node).  A singular problem
 * is refused (CHEBHIP_ERR_ARG).  x may not alias f or g, u_full none of them.  The first solve, and a solve whose restart length
 * differs from the one before, allocates the Krylov bases (see cheb_varhelm_create). */
int  cheb_varhelm_solve(cheb_varhelm *h, const double *f_dev, const double *g_dev, double *x_dev, int x_nonzero, double *u_full_dev,
                        double rtol, double atol, int max_it, int restart, void *stream);
int  cheb_varhelm_iterations(const cheb_varhelm *h);      /* of the last solve, as chebhip_fgmres_* */
double cheb_varhelm_last_residual(const cheb_varhelm *h);
int  cheb_varhelm_reason(const cheb_varhelm *h);

/* The deflated solve of a singular handle.  With c == 0 and every direction periodic or Neumann / Neumann the null
 * space of mult is known for any kappa: the products over the directions of the constant and, on a periodic direction of even
 * extent, the Nyquist vector (-1)^j -- q = 2^(even periodic directions) mutually orthogonal vectors z_1 .. z_q of +-1 in the
 * unknown layout, N = [z_1 .. z_q], N^T N = G I (G unknowns per field).  Pi = I - N N^T / G, per stacked field.
 * cheb_varhelm_solve_deflated returns x with N^T x = 0 and Pi (b - A x) = 0, b = residual(0, f, g): FGMRES on v -> Pi A v from
 * Pi b and the guess Pi x, right preconditioner r -> Pi H(0)^-1 (r / kappa), one last Pi on x, u_full the extension of that x.
 * What is left of b - A x is N lambda, the source the discrete problem cannot balance (collocation has no exact compatibility
 * condition).  iterations, last_residual and reason are those of the projected system: |Pi (b - A x)| against rtol |Pi b|.
 * On a nonsingular handle the call is cheb_varhelm_solve: the same launches, the same bits.  More than three even periodic
 * directions (q > 8): CHEBHIP_ERR_ARG.  Arguments, aliasing rules and the Krylov bases as cheb_varhelm_solve. */
int  cheb_varhelm_solve_deflated(cheb_varhelm *h, const double *f_dev, const double *g_dev, double *x_dev, int x_nonzero, double *u_full_dev,
                                 double rtol, double atol, int max_it, int restart, void *stream);
/* q of the handle as its coefficients stand: 0 where it is not singular; -1: NULL, no coefficients yet, or q > 8 */
int  cheb_varhelm_null_count(const cheb_varhelm *h);
/* lambda = N^T (b - A x) / G of the last deflated solve of a singular problem, nfields x q values to the HOST; from one residual
 * at the end of that solve.  Synchronises the device.  CHEBHIP_ERR_ARG where no such solve has run. */
int  cheb_varhelm_defect(cheb_varhelm *h, double *out);
/* The null vectors of a geometry (HOST, no device): flags[j], j < q, has bit k set where vector j alternates, (-1)^index, in
 * direction k; flags[0] = 0 is the constant, and vector j's directions are the bits of j over the even periodic directions in
 * ascending order.  flags: 8 ints.  Returns q, or -CHEBHIP_ERR_ARG with the error set (q > 8 among the reasons). */
int  cheb_varhelm_null_signs_host(int d, const int *dims, const int *basis, int *flags);
/* out = Pi in, three launches and no allocation: the q signed sums and sum |in| per field as block shares in a fixed order, their
 * totals, the subtraction.  A field whose every |z_j^T in| is at most (q + 4) 2^-53 sum |in| is left bit for bit as it is: Pi
 * could bring it no closer to its range.  out may be in.  The identity on a nonsingular handle.  Results repeat bit for bit. */
int  cheb_varhelm_remove_null(cheb_varhelm *h, const double *in_dev, double *out_dev, void *stream);
/* Pi mult and Pi precond with the shape of chebhip_apply_fn (ctx = the handle): a caller's chebhip_fgmres_solve on the two from
 * b = remove_null(residual(0, f, g)), followed by remove_null of its x, gives cheb_varhelm_solve_deflated's bits. */
int  cheb_varhelm_apply_deflated(void *h, const double *x_dev, double *y_dev, void *stream);
int  cheb_varhelm_precond_deflated(void *h, const double *r_dev, double *z_dev, void *stream);

/* The variable-density projection: out_k = u_k - kappa s_k d_k phi at every node, kappa = 1 / rho > 0 one full-grid
 * field shared by the vectors, phi from
 *   unknown nodes:   sum_k s_k^2 d_k( kappa d_k phi ) = sum_k s_k d_k u_k
 *   boundary node b (k the highest direction in which b is an end node):
 *     wall:  kappa s_k dphi/dnu = +- u_k - flux_b      open:  phi = 0
 * so that the normal velocity of the result at a wall node is flux, as for cheb_project_apply.  The handle of
 * cheb_project_create_variable (arguments of cheb_project_create_basis; basis NULL: no periodic direction) owns a cheb_varhelm
 * (nvec fields, c = 0, (0, 1) ends at walls and (1, 0) at open faces) in place of the direct solve, the unknowns of its last solve
 * and d work grids per vector.  cheb_project_set_inverse_density is cheb_varhelm_set_coefficients(kappa, c = 0): synchronous, and a
 * refused kappa leaves the handle as it was.  cheb_project_apply_variable: the divergence into phi; one launch for f = -div u and
 * g = (+- u_k - flux) / kappa (the operator's faces carry no kappa); cheb_varhelm_solve_deflated with rtol, atol, max_it, restart,
 * from 0 or -- warm != 0 and an earlier call has solved -- from that call's unknowns, the full grid into phi; the gradient of phi
 * (d sweeps per vector), at the nodes of a wall the normal derivative +-g from the condition that defines phi there, and one
 * pointwise pass.  Arrays and aliasing as cheb_project_apply; nothing is allocated per call after the
 * first solve's Krylov bases; the same input gives the same bits.
 * At the unknown nodes div(out) = -cheb_varhelm_residual(phi, -div u, g) exactly as computed: with an open face it is at the
 * solve's tolerance (not at rounding, as the direct solve's is); with walls and periodic directions only it lies in the span of
 * the null vectors up to that tolerance, with the coefficients -cheb_varhelm_defect.  cheb_project_varhelm: the inner handle, for
 * cheb_varhelm_iterations, _last_residual, _reason, _null_count and _defect (NULL for a handle of the other constructors, which
 * cheb_project_apply_variable refuses, as cheb_project_apply refuses a variable one). */
int  cheb_project_create_variable(int d, const int *dims, const int *basis, const int *faces, const double *scale, int nvec, cheb_project **out);
int  cheb_project_set_inverse_density(cheb_project *h, const double *kappa_dev, void *stream);
int  cheb_project_apply_variable(cheb_project *h, const double *u_dev, const double *flux_dev, double *phi_dev, double *out_dev, int warm,
                                 double rtol, double atol, int max_it, int restart, void *stream);
cheb_varhelm *cheb_project_varhelm(const cheb_project *h);

/* ------------------------------------------------------------------------- */
/* Instrumentation (the reference has none: SURVEY 5.1).                      */
/* ------------------------------------------------------------------------- */
/* Run-time options: named integer switches, process-wide, read where they apply (the library never reads the
 * environment).  Unknown names are an error.  Set them before creating the handles they concern.
 *   general_kernels       1: every sweep runs the general 8-byte kernel (A/B against the 16-byte kernels); the preconditioner's
 *                            forward line transforms then run as dense line products
 *   separate_launches     1: the d sweeps of a Stokes gradient / divergence are d launches instead of one
 *   vendor_gemm           1: plain sweeps of lines of more than 1024 points go to rocBLAS DGEMM (looked up at run time, never linked)
 *                            instead of the library's own FP64-VALU kernel.  Default 0: no vendor GEMM on any default path
 *   no_raw_transforms     1: the preconditioner's line transforms run as a dense line product (forward) / two launches (backward)
 *                            instead of one raw-mode launch
 *   equal_shares          1: multi-job launches give every job min(tiles, CUs) workgroups instead of proportional shares
 *   force_gemm            1: every extent of 4 .. 256 points takes the library-DGEMM route of the longest lines (read at operator create)
 *   stokes_single_stream  1: StokesMatMult / StokesFunction keep the pressure chain on the caller's stream, also on large grids off the
 *                            fused-z route (read at create)
 *   eta_from_memory       1: FormFunction reads eta instead of forming 1 + gamma u^2 on chip (exponent 2)
 *   gather_pass           1: FormFunction always runs its gather pass, also for homogeneous Dirichlet rows
 *   rccl_self_messages    1: a rank's own block of an exchange goes through ncclSend / ncclRecv too (one-rank smoke runs)
 *   local_timeout_s       seconds a thread rank (LOCAL) or process rank (IPC: barrier and polling launch) waits for its peers before the group is aborted (default 120)
 *   dist_single_stream    chebhip_dist_mult's local sweeps: 0 (default) = by transport -- on a side stream (they overlap both exchanges) when
 *                            data leaves the device (RCCL, a callback transport, thread ranks on several devices), on the caller's stream
 *                            when it does not (one rank, the NULL transport, thread ranks sharing one device: there the side stream only
 *                            adds dependencies and costs 8-27 %); 1 = always the caller's stream; 2 = always the side stream
 *   dist_packed_exchange  1: chebhip_dist_mult on a direct transport (LOCAL thread ranks, NULL) runs pack / segment exchange / final sum
 *                            as on RCCL instead of reading the peers' slabs and pencil results in place; 2: in place, but the pencil is
 *                            filled by a copy launch first instead of the pencil sweep reading the peers' slabs itself; 3: the pencil
 *                            sweep reads the peers' slabs but stays a launch of its own (default on a small slab: one launch of the three
 *                            directions); 4: the pencil results stay where they are computed and the final sum reads the peers' (default:
 *                            the pencil sweep stores every output row into the result array of the rank that owns the plane, the final
 *                            sum reads local memory) (A/B and tests; set it before the first matvec of a handle, on every rank)
 *   long_lines_gemm       1: lines of 257 .. 1024 points go to rocBLAS instead of the library's own matrix-core kernel (A/B)
 *   pressure_passes       1: Stokes handles run the three boundary-extrapolation passes of StokesPressureReduceOrder before the
 *                            pressure gradient instead of folding each direction's extrapolation into its matrix (read at create)
 *   general_viscous       1: StokesMatMult / StokesMatMultVV take the general viscous block also when the viscosity is uniform and
 *                            eta' = 0 (linear rheology), instead of -eta/2 (sum_j D_j D_j v + grad div v) (read at create)
 *   poisson_launches      the constant-coefficient MatMult_Elliptic: 0 = by size (below 6 M unknowns: from 1.5 M on, in 3-D with lines of at most 128 points, two
 *                            jobs in one launch and a last direction that adds both terms as it stores, otherwise one launch of d jobs + a sum;
 *                            above: in 3-D, while the padded field has at most 9 M values, two jobs in one launch + a last direction that adds
 *                            both terms; otherwise a launch per direction), 1 = always the d-job launch (below 6 M unknowns), 2 = always a
 *                            launch per direction, 3 = the two-launch form at every large 3-D size (A/B: it loses from 240^3 on)
 *   dist_exact_order      1: chebhip_dist_mult adds its terms in the serial order V = ((T_0 + A_1) + A_2) (elliptic.C:331-334), which
 *                            reproduces the one-GPU vector to the bit; 0 (default): the local terms are accumulated into one array
 *                            by the sweeps themselves, V = T_0 + (A_1 + A_2) -- equal to rounding, one array less to read
 *   fdm_z_separate        1: the fast-diagonalisation solve runs its last forward line transform, the modal scaling and its first backward
 *                            line transform as separate launches also where the one-launch form exists (last dimension with 66 .. 128
 *                            interior points, an even number) (A/B)
 *   stokes_z_separate     1: StokesMatMult / StokesMatMultVV / StokesFunction run the z direction of the viscous block as separate passes
 *                            (z sweeps of the gradient launch, node loop, z sweeps of the divergence launch) also where the one-launch
 *                            form exists (d = 3 on one GPU, contiguous lines of 68 .. 128 points, at least 14 400 of them); same bits (A/B)
 *   saddle_node_major     1: the block preconditioners (stokes_saddle_*) keep the vectors of their inner velocity solves node-major as
 *                            the reference does, with a (de)interleaving pass around every MatVVPC solve (read at create; A/B)
 *   fdm_passes            1: the fast-diagonalisation solve z = P_1^-1 (r / eta) of the finite-difference preconditioners divides by eta
 *                            and by the modal sums in passes of their own, instead of multiplying by the reciprocals in the load of its
 *                            first and the store of its last forward line transform (A/B; the two differ in the last bits)
 *   full_stress_storage   1: Stokes handles keep all 9 stress / strain components instead of the 6 distinct ones (read at create)
 *   stokes_pressure_stream 1: where the fused-z route runs, the pressure-gradient sweeps go to a second stream between the gather and the
 *                            final scatter (rounds 2-4) instead of being jobs of the route's first launch (read at create; A/B: a tie)
 *   stokes_pressure_sweeps 1: where the fused-z route runs, StokesMatMult / StokesFunction run the three pressure-gradient sweeps and add grad p in
 *                            the final scatter (rounds 1-4), instead of subtracting the pressure -- face values extrapolated along each line, one
 *                            small launch -- from the diagonal stress so that the three divergence sweeps deliver -div tau + grad p at once
 *                            (read per call; A/B: the two agree to rounding, 4e-16 observed)
 *   krylov_exact_norm     1: chebhip_fgmres runs its Gram-Schmidt step as three launches with an explicit norm pass (rounds 1-4) instead of
 *                            two launches with one reduction and the stored vectors' exact norms carried beside the basis (read per solve; A/B)
 *   points_spread_pass    cheb_points_spread: at most this many points per pass; 0 (default) = as many as the handle's work memory holds
 *                            rows for (read per call; tests reach the multi-pass path at small counts with it)
 *   sweep_alpha_multiply  1: the long-line STORE sweep with alpha = -1 on a symmetric line operator multiplies by alpha as every other launch
 *                            does, instead of carrying the sign in its recombination (read per launch; A/B, the same values)
 *   no_rocblas            deprecated alias (rounds 1-3) of vendor_gemm with the inverted meaning; still accepted */
int chebhip_set_option(const char *name, int value);
int chebhip_get_option(const char *name, int *value);
const char *chebhip_option_name(int index);     /* "" past the last option: enumerate from 0 */

/* Number of sweep-kernel launches issued by this process so far. */
long chebhip_launch_count(void);
/* ... and how many of them ran the 16-byte line kernels (csrc/sweep_vec.hip) rather than the general kernel or a long-line route:
 * kernel selection is silent, this is how a caller sees it. */
long chebhip_vec_launch_count(void);

/* Per-stage device timers: when enabled, every entry point listed below brackets its work with a hipEvent pair on
 * the caller's stream (inclusive times: stokes_saddle_apply contains the stokes_op_mult_vv calls of its inner
 * solves).  Reading drains the pending events (synchronises with them).  Off by default: no events, no cost. */
enum {
  CHEBHIP_STAGE_CHEB_APPLY = 0, CHEBHIP_STAGE_ELL_MULT, CHEBHIP_STAGE_ELL_FUNCTION, CHEBHIP_STAGE_STOKES_MULT,
  CHEBHIP_STAGE_STOKES_MULT_VV, CHEBHIP_STAGE_STOKES_MULT_PV, CHEBHIP_STAGE_STOKES_MULT_VP, CHEBHIP_STAGE_STOKES_FUNCTION,
  CHEBHIP_STAGE_STOKES_SCHUR, CHEBHIP_STAGE_FDPC_APPLY, CHEBHIP_STAGE_SADDLE_APPLY, CHEBHIP_STAGE_FGMRES_SOLVE,
  CHEBHIP_NSTAGES
};
int chebhip_timers_enable(int on);
int chebhip_timers_reset(void);
int chebhip_timers_read(int stage, double *total_ms, long *calls);
const char *chebhip_stage_name(int stage);

/* min / max of the viscosity left by the last stokes_op_function: the VecMin / VecMax the reference prints inside
 * StokesFunction (stokes.C:731-734).  Synchronises with `stream`; never called implicitly. */
int stokes_op_viscosity_range(stokes_op *op, double *eta_min, double *eta_max, void *stream);
/* StokesStateView (stokes.C:1821-1894, -output_vtk): legacy ASCII VTK file with velocity, pressure, force, eta, deta and
 * strain on the full grid, same sections and number format as the reference.  Host I/O; synchronises the device. */
int stokes_op_write_vtk(stokes_op *op, const double *state_dev, const char *path);

#ifdef __cplusplus
}
#endif
#endif
