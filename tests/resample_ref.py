"""Reference side of the per-element checks of Resample, the two prolongations of solve.py and the ChebModal tensor products
(helper module of test_resample_elementwise_host.py, test_gpu_resample.py and test_gpu_modal.py; no device).

A call is a chain of line products, one per direction that runs (not the identity, not dropped).  In direction k, K_k stored input
points are multiplied by the DOUBLE matrix A_k the library itself builds on the host.  To first order, for every output element i,

    |y_i - truth_i| <= cap 2^-53 B_i,     cap = sum_k (K_k + 8) over the directions that run,
    B = (x_k |A_k|) |x|,                  truth = (x_k A_k) x in long double from the double matrices.

K_k + 8 per product as in linewise.py: one rounding per matrix entry, K_k for the sum in any order, a few spare; the rounding of an
intermediate is one of the spare ones of the next product.  The |A_k| of different directions commute, so B does not depend on the
order in which the directions run.  B_i = 0 demands an exact zero (linewise.worst); no running direction demands the input's bits."""
import functools

import numpy as np

import __graft_entry__ as ge
import linewise as lw

sp = ge.load()
LD = np.longdouble
KINDS = ("noise", "scaled", "impulse", "alternating", "constant")


def stored(dims, nodes):
    """Stored points per direction of the node set."""
    return tuple(n - 2 if nodes == "interior" else n for n in dims)


@functools.lru_cache(maxsize=None)
def mats(dims_in, dims_out, nodes_in, nodes_out):
    """The library's double interpolation matrix of every direction, (stored out, stored in)."""
    out = tuple(sp.resample_matrix(a, b, nodes_in, nodes_out) for a, b in zip(dims_in, dims_out))
    for M in out:
        M.setflags(write=False)
    return out


def runs(M):
    """cheb_resample_create's rule: a direction is skipped when its stored sizes are equal and its diagonal is all ones (the rows
    are unit rows then); None stands for a dropped direction of ChebModal."""
    if M is None:
        return False
    return not (M.shape[0] == M.shape[1] and bool((np.diagonal(M) == 1.0).all()))


def run_order(Ms):
    """The running directions in the order the library runs them (order_by_ratio: ascending out / in, stable)."""
    key = functools.cmp_to_key(lambda a, b: -1 if Ms[a].shape[0] * Ms[b].shape[1] < Ms[b].shape[0] * Ms[a].shape[1] else
                               (1 if Ms[b].shape[0] * Ms[a].shape[1] < Ms[a].shape[0] * Ms[b].shape[1] else 0))
    return sorted((k for k, M in enumerate(Ms) if runs(M)), key=key)


def chain(Ms, x, order=None, first_axis=0, dtype=np.float64):
    """The matrices applied along the axes first_axis + k of x, one direction after the other in `order` (default: ascending), in
    `dtype`: long double is the truth, float64 what a plain IEEE implementation gives."""
    t = np.asarray(x).astype(dtype)
    for k in (range(len(Ms)) if order is None else order):
        if Ms[k] is not None:
            t = np.moveaxis(np.tensordot(np.asarray(Ms[k]).astype(dtype), t, axes=([1], [first_axis + k])), 0, first_axis + k)
    return t


def chain_truth_bound(Ms, x, first_axis=0, skip_identities=True):
    """(truth, B, cap) of a list of matrices (None: a dropped direction) along the axes first_axis .. of x: fields outermost with
    first_axis = 1, the ChebModal layout.  skip_identities: Resample's rule (`runs`) decides which directions run and count, their
    matrices being exact identities; otherwise (ChebModal) every matrix that is not None does."""
    live = [M if (runs(M) if skip_identities else M is not None) else None for M in Ms]
    with np.errstate(invalid="ignore"):
        B = chain([None if M is None else np.abs(M) for M in live], np.abs(x), first_axis=first_axis)
    return chain(live, x, first_axis=first_axis, dtype=LD), B, sum(M.shape[1] + 8 for M in live if M is not None)


def truth_bound(x, dims_in, dims_out, nodes_in="all", nodes_out="all"):
    """(truth, B, cap) of a Resample call on x of shape stored(dims_in) + (ncomp,)."""
    return chain_truth_bound(mats(tuple(dims_in), tuple(dims_out), nodes_in, nodes_out), x)


# ----------------------------------------------------------------------------------------------
# inputs in the (... stored dims, ncomp) layout
# ----------------------------------------------------------------------------------------------
def long_axis(shape):
    """The direction with the most stored points (the first of them)."""
    return int(np.argmax(shape[:-1]))


def inputs(kind, shape, seed, order=None):
    """The arrays of one input kind for a tensor of `shape` = stored dims + (ncomp,); every kind is one array but `impulse`.
      noise        N(0, 1);
      scaled       N(0, 1) times 10^e, e the integers nearest to evenly spaced values over [-100, 100], one per scale, in seeded
                   random order (so two scales are 10^-100 and 10^100, never two alike).  `order` lists the directions that run, in run order (None:
                   all of them, in index order).  e is drawn per component and per index of every direction that does not run:
                   with one running direction that is one scale per line of the direction under test (linewise.scaled), so
                   that neighbouring lines of a tile differ by up to 10^200 and no line mixes scales.  A chain of two or more
                   running directions has no index left that is never contracted but the component's, so there e varies along
                   the direction that runs last as well: every earlier product sees lines of one scale each, only the last
                   one mixes them.  No product overflows: the matrices' entries are far below 10^100;
      impulse      three combs of 1.0 at the multi-indices with (sum of indices + component + s) % 3 == 0, s = 0, 1, 2: every
                   column of every direction's matrix multiplies a 1.0 in at least one of them, all other operands are exact zeros;
      alternating  (-1)^j along the longest direction times an N(0, 1) constant per line: the largest outputs a row can produce;
      constant     one N(0, 1) constant per component: reproduced, since interpolation rows sum to 1."""
    shape = tuple(shape)
    d = len(shape) - 1
    if kind == "noise":
        return [lw.noise(shape, 0, seed)]
    if kind == "scaled":
        order = list(range(d)) if order is None else list(order)
        es = [1 if k in order else shape[k] for k in range(d)] + [shape[-1]]
        if len(order) > 1:
            es[order[-1]] = shape[order[-1]]
        n = int(np.prod(es))
        rng = np.random.default_rng(seed + 1)
        e = rng.permutation(np.rint(np.linspace(-100, 100, n)).astype(np.int64)).reshape(es) if n > 1 else rng.integers(-100, 101, size=es)
        return [lw.noise(shape, 0, seed) * 10.0 ** e]
    if kind == "impulse":
        s = sum(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij", sparse=True))
        return [((s + k) % 3 == 0).astype(np.float64) for k in range(3)]
    if kind == "alternating":
        return [lw.alternating(shape, long_axis(shape), seed)]
    if kind == "constant":
        return [np.random.default_rng(seed).standard_normal((1,) * d + (shape[-1],)) * np.ones(shape)]
    raise ValueError(kind)


def unit_impulses(K, ncomp, run):
    """Input `run` of the bit-for-bit check of a one-direction handle: component c holds a single 1.0 at point (run ncomp + c) mod K,
    so ceil(K / ncomp) runs show every column of the matrix.  Returns (x of shape (K, ncomp), the columns)."""
    j = (run * ncomp + np.arange(ncomp)) % K
    x = np.zeros((K, ncomp))
    x[j, np.arange(ncomp)] = 1.0
    return x, j


# ----------------------------------------------------------------------------------------------
# the prolongations of solve.py, from their documented layout
# ----------------------------------------------------------------------------------------------
def interior_mask(dims):
    m = np.zeros(tuple(dims), dtype=bool)
    m[tuple(slice(1, n - 1) for n in dims)] = True
    return m


def full_field(dims, inner, boundary):
    """The full grid field (dims + (ncomp,)) of interior values (row-major over the interior nodes, ncomp innermost) and compact
    boundary values (row-major over the boundary nodes)."""
    m = interior_mask(dims)
    inner = np.asarray(inner, dtype=np.float64)
    ncomp = inner.size // int(m.sum())
    full = np.empty(tuple(dims) + (ncomp,))
    full[m] = inner.reshape(-1, ncomp)
    full[~m] = np.asarray(boundary, dtype=np.float64).reshape(-1, ncomp)
    return full


def prolong_elliptic(dims_c, x_c, dirichlet_c, dims_f):
    """(truth, B, cap) of solve.prolong_elliptic, shape stored(dims_f, interior) + (1,): the full coarse field ALL -> INTERIOR."""
    return truth_bound(full_field(dims_c, x_c, dirichlet_c), dims_c, dims_f, "all", "interior")


def prolong_stokes(dims_c, x_c, dirichlet_c, dims_f):
    """((truth, B, cap) of the velocity, (truth, B, cap) of the pressure) of solve.prolong_stokes; the state holds
    [v_0 .. v_{d-1}, p] per interior node, the result's velocity is out[..., :d], its pressure out[..., d:]."""
    d = len(dims_c)
    xc = np.asarray(x_c, dtype=np.float64).reshape(-1, d + 1)
    vel = truth_bound(full_field(dims_c, xc[:, :d], dirichlet_c), dims_c, dims_f, "all", "interior")
    p = np.ascontiguousarray(xc[:, d]).reshape(stored(dims_c, "interior") + (1,))
    return vel, truth_bound(p, dims_c, dims_f, "interior", "interior")


def grid(dims, nodes):
    """Node coordinates of the stored nodes, one sparse array per direction."""
    ax = [np.cos(np.pi * np.arange(n) / (n - 1))[1:n - 1] if nodes == "interior" else np.cos(np.pi * np.arange(n) / (n - 1))
          for n in dims]
    return np.meshgrid(*ax, indexing="ij", sparse=True)


def cubic(g, c=0):
    """A polynomial of degree 3 in the first direction, 2 in the second and 3 in the last one (a grid of 4 points per direction
    holds it), one per component c."""
    return (1.0 + c) + g[0] ** 3 - (2.0 + c) * g[0] * g[1 % len(g)] ** 2 + 0.5 * g[-1] ** 3 + 0.0 * sum(g)


def bilinear(g):
    """Degree 1 per direction: what the pressure's two interior nodes of a 4-point direction hold."""
    return 1.0 + g[0] * g[1 % len(g)] - 0.5 * g[-1] + 0.0 * sum(g)


def split(field, dims):
    """(interior values row-major, compact boundary values row-major) of a full field dims + (ncomp,)."""
    m = interior_mask(dims)
    return field[m].ravel(), field[~m].ravel()


def elliptic_polynomial(dims_c, dims_f):
    """(x_c, dirichlet_c, the polynomial on the fine interior) of the degree-3 state."""
    x, dv = split(cubic(grid(dims_c, "all"))[..., None], dims_c)
    return x, dv, cubic(grid(dims_f, "interior"))[..., None]


def stokes_polynomial(dims_c, dims_f):
    """(x_c, dirichlet_c, velocity on the fine interior, pressure on the fine interior): cubic velocity components with their own
    boundary values, a pressure of degree 1 per direction."""
    d = len(dims_c)
    v = np.stack([cubic(grid(dims_c, "all"), c) for c in range(d)], axis=-1)
    vin, dv = split(v, dims_c)
    p = bilinear(grid(dims_c, "interior"))
    x = np.concatenate([vin.reshape(-1, d), p.reshape(-1, 1)], axis=1).ravel()
    return (x, dv, np.stack([cubic(grid(dims_f, "interior"), c) for c in range(d)], axis=-1),
            bilinear(grid(dims_f, "interior"))[..., None])


# ----------------------------------------------------------------------------------------------
# the shapes of the per-element tests: the smallest at which a route of cheb_resample_kernel or line_chain changes;
# (dims_in, dims_out, nodes_in, nodes_out, ncomp), grouped by what they reach
# ----------------------------------------------------------------------------------------------
_A, _I = "all", "interior"
SHAPES = {
    # chunks of 16 contracted points: K = 2, 15, 16, 17, 33; one stored point in (K = 1) and out (M = 1)
    "chunks": [((2,), (7,), _A, _A, 1), ((15,), (9,), _A, _A, 1), ((16,), (24,), _A, _A, 1), ((17,), (33,), _A, _A, 1),
               ((33,), (20,), _A, _A, 1), ((3,), (7,), _I, _I, 1), ((9,), (3,), _A, _I, 1)],
    # output tile of 64 / 128 points and grid.y: M = 63, 64, 65, 128, 129 from K = 20; the 1024-point limits
    "tile": [((20,), (m,), _A, _A, 1) for m in (63, 64, 65, 128, 129)] +
            [((2,), (1024,), _A, _A, 1), ((1024,), (3,), _A, _A, 1), ((1024,), (700,), _I, _A, 1)],
    # line tile of 64 and the o = line / Q split: a middle direction with O > 1 and Q > 1, L = O Q = 63, 64, 65, 130 (L = 1: "chunks")
    "lines": [((7, 12, 9), (7, 17, 9), _A, _A, 1), ((8, 12, 8), (8, 17, 8), _A, _A, 1), ((5, 12, 13), (5, 17, 13), _A, _A, 1),
              ((10, 12, 13), (10, 17, 13), _A, _A, 1)],
    # LINES_A (Q <= 4): the last direction with 1 .. 4 components at M <= 64 and M > 64; a non-last direction at Q = 4
    "lines_a": [((5, 20), (5, m), _A, _A, c) for c in (1, 2, 3, 4) for m in (33, 70)] + [((12, 2), (17, 2), _A, _A, 2)],
    # one direction alone with 2, 3 and 4 components (the lines are the components: Q = ncomp, O = 1), at M <= 64, M > 64 and K = 1024
    "components": [((1024,), (3,), _A, _A, 2), ((20,), (33,), _A, _A, 3), ((20,), (70,), _I, _A, 4)],
    # COLFAST (Q > 4) at Q = 5 (the first), 15, 16, 17, and at M > 64
    "colfast": [((12, q), (17, q), _A, _A, 1) for q in (5, 15, 16, 17)] + [((20, 6), (70, 6), _A, _A, 1)],
    # node sets: the four combinations at d = 2 and 3 with 3 components; one stored point in, then out, in different directions
    "nodes": [(di, do, a, b, 3) for di, do in (((7, 6), (9, 8)), ((6, 5, 7), (8, 9, 6))) for a in (_A, _I) for b in (_A, _I)] +
             [((3, 5), (7, 3), _I, _I, 1)],
    # chains of 2 .. 5 running directions (one: everything above); an identity direction in the middle; five directions of
    # which two shrink and three grow, so that both work buffers are written twice and the run order is not the index order
    "chains": [((9, 7), (16, 5), _A, _A, 2), ((6, 5, 4, 3), (7, 9, 4, 5), _A, _A, 1), ((6, 5, 7, 4), (8, 4, 9, 6), _A, _A, 1),
               ((9, 4, 8, 5, 6), (5, 7, 4, 9, 11), _A, _A, 2)],
}
ALL_SHAPES = [s for group in SHAPES.values() for s in group]


def shape_id(s):
    di, do, a, b, c = s
    return "%s%s-%s%s-c%d" % ("x".join(map(str, di)), a[0], "x".join(map(str, do)), b[0], c)


def geometry(s):
    """[(direction, O, K, M, Q)] of the launches of a shape in run order, as line_chain forms them: O outer lines, Q the stride
    of the contracted index (components included)."""
    di, do, a, b, c = s
    Ms = mats(tuple(di), tuple(do), a, b)
    cur = list(stored(di, a))
    out = []
    for k in run_order(Ms):
        O = int(np.prod(cur[:k], dtype=np.int64))
        Q = int(np.prod(cur[k + 1:], dtype=np.int64)) * c
        out.append((k, O, cur[k], Ms[k].shape[0], Q))
        cur[k] = Ms[k].shape[0]
    return out


def route(K, M, Q):
    """resample_launch's rule: (LINES_A, BM)."""
    return Q <= 4, 128 if M > 64 else 64
