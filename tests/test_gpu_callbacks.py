"""The Stokes callbacks (stokes.hip) and the variable-coefficient EllipticOp callbacks (fused4.hip, fused.hip, chebhip.hip),
element by element, against the long-double truths of the oracle (run with -m gpu on the MI355X box).  The bar, for EVERY output
element, velocity rows and pressure rows separately:

    |y_i - truth_i| <= cap 2^-53 W_i          (W_i = 0 demands y_i == 0 exactly)

W and the caps are derived in tests/callbacks_ref.py ("Per-element bar: callbacks"): cap_v = 2 (K + 8) + d^2 + d + 6,
cap_p = K + 8 + d, K the longest line.  Every case prints `callback-ratio <test id> <input> <worst ratio> at <index> cap <cap>`;
profiles/callbacks/ratios.txt holds the lines of a run on an MI355X.

Which kernels a shape runs is decided by the library (stokes.hip: stokes_op_create, st_zfused_ok, st_fold_pressure, st_out_pairs,
st_local); the ABI reports launch counts only, which do not name kernels.  `routes()` restates the dispatch conditions and
test_route_rules asserts, on the shapes below, that each reaches the route it is listed for:

  (20, 17)        d = 2: scalar node and scatter kernels (k_st_node_vv<2>, k_st_local, k_st_out)
  (13, 11, 9)     d = 3, N odd: scalar node kernels, k_st_local4 / k_st_out4
  (14, 12, 9)     N even, last extent odd: pair kernels, interior index from the table
  (14, 12, 10)    pair kernels, arithmetic interior index
  (66, 96, 66)    the six-slot stress storage T (all extents even and >= 66; 66 * 96 lines are a multiple of 64)
  (120, 121, 68)  fused z launch (14 520 z lines >= 14 400) without T (121 is odd); the last tile of 16 lines is partial
  (120, 120, 68)  fused z launch with T, the pressure folded into the stress; again with stokes_pressure_sweeps = 1 and with the
                  result vector at an 8-byte offset (st_fold_pressure then refuses: the pressure-gradient sweeps)
  (98, 96, 130)   two streams (N = 1 223 040 >= 1.2 M, no fused z: 130 > 128); KS = 32 lines

States: the default (eta = 1: the uniform-viscosity route on D D matrices), the default with general_viscous = 1, a variable eta
with eta' = 0, and eta, eta', symmetric S0 all set.  Inputs: callbacks_ref.py (noise, blocks, node-scaled, constant pressure,
impulses).  The dependence and recovery tests put NaN / +Inf into the input and compare bits.

Measured on an MI355X: velocity rows at most 10.8 (caps 62 .. 294), pressure rows at most 8.7 (caps 24 .. 141), strain 7.0,
EllipticOp 8.9 (caps 47 .. 287), eta and eta' at most 0.12 of their bound, the device pow 1.32 ulps; 216 tests in 135 s, the slowest
case (impulses at 98 x 96 x 130, full state) 6 s."""
import math

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import callbacks_ref as cb
import linewise as lw
import oracle_lib as orc

pytestmark = pytest.mark.gpu
sp = ge.load()
NT = 16
POWER = (1, 1.0, 3.0, 1e-2, 1.0)
LINEAR = (0, 1.0, 1.0, 1.0, 1.0)
SMALL = [(20, 17), (13, 11, 9), (14, 12, 9), (14, 12, 10)]
LARGE = [(66, 96, 66), (120, 121, 68), (120, 120, 68), (98, 96, 130)]
GPU_STATES = ("default", "general", "eta", "full")
FAMILIES = ("noise", "scaled", "constant-pressure", "impulses")
CM_SHAPES = [(14, 12, 10), (120, 120, 68)]
ELL_SHAPES = [(24, 20), (12, 11, 10), (33, 40), (130, 66), (20, 129, 18), (68, 70, 72), (132, 68, 130)]
ELL_OPTIONS = (None, "general_kernels", "separate_launches", "eta_from_memory", "gather_pass")
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)
_NODE = [""]
_OPS = {}
_TRUTH = {}


@pytest.fixture(autouse=True)
def _nodeid(request):
    _NODE[0] = request.node.nodeid.split("::", 1)[-1]
    yield


@pytest.fixture(scope="module", autouse=True)
def _handles():
    yield
    for op in _OPS.values():
        op.destroy()
    _OPS.clear()
    _TRUTH.clear()


def record(kind, r, idx, cap):
    print("callback-ratio %s %s %.2f at %s cap %d" % (_NODE[0], kind, r, idx, cap))


class option:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: sp.get_option(k) for k in self.kw}
        for k, v in self.kw.items():
            sp.set_option(k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            sp.set_option(k, v)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def run(fn, x, nout, offset8=False):
    """fn(x, y) on a NaN-filled result vector; offset8: the result vector starts 8 bytes past a 16-byte boundary."""
    if offset8:
        buf = torch.full((nout + 1,), float("nan"), dtype=torch.float64, device="cuda")
        y = buf[1:]
        assert y.data_ptr() % 16 == 8
    else:
        y = torch.full((nout,), float("nan"), dtype=torch.float64, device="cuda")
        assert y.data_ptr() % 16 == 0
    fn(dev(x), y)
    torch.cuda.synchronize()
    return y.cpu().numpy()


# ----------------------------------------------------------------------------------------------
# the dispatch conditions of stokes.hip, restated
# ----------------------------------------------------------------------------------------------
def ks_of(K):
    ks = 4
    while 4 * ks < (K + 1) // 2:
        ks *= 2
    return ks


def routes(dims, aligned16=True, pressure_sweeps=False):
    d, N = len(dims), int(np.prod(dims))
    r = {"pairs": d == 3 and N % 2 == 0}                                          # k_st_node_vv_pair, k_st_local4p, k_st_out4p
    r["arith"] = r["pairs"] and dims[-1] % 2 == 0                                 # st_grid: P2 != 0
    P = dims[-1]
    r["T"] = (d == 3 and N % 2 == 0 and all(p % 2 == 0 and ks_of(p) >= 16 for p in dims)
              and (N // P) % (64 if ks_of(P) == 16 else 32) == 0)                 # stokes_op_create: op->sym
    r["zfused"] = d == 3 and N % 2 == 0 and 64 < P <= 128 and P % 4 == 0 and N // P >= 14400      # st_zfused_ok
    r["fold"] = r["zfused"] and aligned16 and not pressure_sweeps                 # st_fold_pressure
    r["streams"] = 2 if (N >= 1200000 and not r["zfused"]) else 1                 # stokes_op_create: op->aux
    r["partial"] = d == 3 and (N // P) % 16 != 0
    return r


def test_route_rules():
    R = routes
    assert not R((20, 17))["pairs"]
    assert not R((13, 11, 9))["pairs"]
    assert R((14, 12, 9))["pairs"] and not R((14, 12, 9))["arith"]
    assert R((14, 12, 10))["arith"] and not R((14, 12, 10))["T"] and not R((14, 12, 10))["zfused"]
    assert R((66, 96, 66))["T"] and not R((66, 96, 66))["zfused"] and R((66, 96, 66))["streams"] == 1
    assert R((120, 121, 68))["zfused"] and not R((120, 121, 68))["T"] and R((120, 121, 68))["partial"]
    assert R((120, 120, 68))["zfused"] and R((120, 120, 68))["T"] and R((120, 120, 68))["fold"]
    assert not R((120, 120, 68), pressure_sweeps=True)["fold"] and not R((120, 120, 68), aligned16=False)["fold"]
    assert R((98, 96, 130))["streams"] == 2 and not R((98, 96, 130))["zfused"] and ks_of(130) == 32
    for smaller in ((120, 119, 68), (98, 94, 130)):                              # the large shapes are the smallest on their routes
        assert not R(smaller)["zfused"] and R(smaller)["streams"] == 1


# ----------------------------------------------------------------------------------------------
# handles and truths
# ----------------------------------------------------------------------------------------------
def make_op(dims, state):
    """A fresh StokesOp in one of GPU_STATES ("general": the default state on a handle created with general_viscous = 1)."""
    with option(general_viscous=1 if state == "general" else 0):
        op = sp.StokesOp(dims)
    eta, deta, S0 = cb.stokes_state(dims, "default" if state == "general" else state)
    if eta is not None:
        op.set_state(0, eta)
    if deta is not None:
        op.set_state(1, deta)
        for j in range(len(dims)):
            op.set_state(2 + j, S0[j])
    return op


def get_op(dims, state):
    if (dims, state) not in _OPS:
        _OPS[(dims, state)] = make_op(dims, state)
    return _OPS[(dims, state)]


def truth(dims, state, key, x):
    """orc.stokes_truth, kept for the variants of (120, 120, 68) that meet the same input again."""
    k = (dims, "default" if state == "general" else state, key)
    if k in _TRUTH:
        return _TRUTH[k]
    eta, deta, S0 = cb.stokes_state(dims, "default" if state == "general" else state)
    t = orc.stokes_truth(dims, x, eta, deta, S0, nthreads=NT)
    if dims == (120, 120, 68) and key.startswith(("noise", "constp")):
        _TRUTH[k] = t
    return t


def hold(dims, y, t, W, what, fn=False, power=False):
    for rowk, r, idx, cap in cb.check_stokes(dims, y, t, W, "%s %s" % (ids(dims), what), fn=fn, power=power):
        record("%s/%s" % (what, rowk), r, idx, cap)


def cm(dims, v):
    """node-major velocity vector -> component-major"""
    return np.ascontiguousarray(np.asarray(v).reshape(-1, len(dims)).T).reshape(-1)


def linear_callbacks(op, dims, state, x, name, offset8=False, with_cm=False):
    """mult on [v; p], [v; 0] and [0; p], then mult_vv, mult_pv and mult_vp, each element against the truth."""
    d = len(dims)
    X = x.reshape(-1, d + 1)
    xv, xp = X.copy(), X.copy()
    xv[:, d] = 0.0
    xp[:, :d] = 0.0
    v, p = np.ascontiguousarray(X[:, :d]).reshape(-1), np.ascontiguousarray(X[:, d])
    t, W = truth(dims, state, name, x)
    hold(dims, run(op.mult, x, op.global_size, offset8), t, W, name + ":mult[v;p]")
    tv, Wv = truth(dims, state, name + "/v", xv.reshape(-1))
    hold(dims, run(op.mult, xv.reshape(-1), op.global_size, offset8), tv, Wv, name + ":mult[v;0]")
    tp, Wp = truth(dims, state, name + "/p", xp.reshape(-1))
    hold(dims, run(op.mult, xp.reshape(-1), op.global_size, offset8), tp, Wp, name + ":mult[0;p]")
    (tvv, tpv), (wvv, wpv) = cb.rows(dims, tv), cb.rows(dims, Wv)
    cv, cp = cb.cap_v(dims), cb.cap_p(dims)
    record(name + ":mult_vv", *lw.check(run(op.mult_vv, v, op.velocity_size, offset8).reshape(-1, d), tvv, wvv, cv, "mult_vv"), cv)
    record(name + ":mult_pv", *lw.check(run(op.mult_pv, v, op.pressure_size, offset8), tpv, wpv, cp, "mult_pv"), cp)
    tvp, wvp = cb.rows(dims, tp)[0], cb.rows(dims, Wp)[0]
    record(name + ":mult_vp", *lw.check(run(op.mult_vp, p, op.velocity_size, offset8).reshape(-1, d), tvp, wvp, cv, "mult_vp"), cv)
    if with_cm:
        record(name + ":mult_vv_cm", *lw.check(run(op.mult_vv_cm, cm(dims, v), op.velocity_size), cm(dims, tvv), cm(dims, wvv), cv, "mult_vv_cm"), cv)
        record(name + ":mult_pv_cm", *lw.check(run(op.mult_pv_cm, cm(dims, v), op.pressure_size), tpv, wpv, cp, "mult_pv_cm"), cp)
        record(name + ":mult_vp_cm", *lw.check(run(op.mult_vp_cm, p, op.velocity_size), cm(dims, tvp), cm(dims, wvp), cv, "mult_vp_cm"), cv)


def family(op, dims, state, fam, offset8=False, with_cm=False):
    d = len(dims)
    if fam == "noise":
        linear_callbacks(op, dims, state, cb.noise(dims, 11), "noise", offset8, with_cm)
    elif fam == "scaled":
        linear_callbacks(op, dims, state, cb.node_scaled(dims, 15), "node-scaled", offset8, with_cm)
    elif fam == "constant-pressure":
        x = cb.constant_pressure(dims, 14)
        t, W = truth(dims, state, "constp", x)
        t = cb.exact_zero(dims, t, W)
        hold(dims, run(op.mult, x, op.global_size, offset8), t, W, "constant-pressure:mult")
        p = np.ascontiguousarray(x.reshape(-1, d + 1)[:, d])
        cv = cb.cap_v(dims)
        record("constant-pressure:mult_vp", *lw.check(run(op.mult_vp, p, op.velocity_size, offset8).reshape(-1, d), cb.rows(dims, t)[0],
                                                      cb.rows(dims, W)[0], cv, "mult_vp"), cv)
    else:
        # one 1.0 per call, call after call on the one handle; small grids: every component at every position, large ones: the
        # components in turn
        small = int(np.prod(dims)) < 100000
        worst = {"v": (0.0, None, cb.cap_v(dims)), "p": (0.0, None, cb.cap_p(dims))}
        for n, node in enumerate(cb.impulse_positions(dims)):
            for c in (range(d + 1) if small else [n % (d + 1)]):
                x = cb.impulse(dims, node, c)
                t, W = truth(dims, state, "impulse", x)
                for rowk, r, idx, cap in cb.check_stokes(dims, run(op.mult, x, op.global_size, offset8), t, W,
                                                         "%s impulse at %s/%d" % (ids(dims), node, c)):
                    if r >= worst[rowk][0]:
                        worst[rowk] = (r, (node, c, idx), cap)
        for rowk, (r, where, cap) in worst.items():
            record("impulses:mult/%s" % rowk, r, where, cap)


# ----------------------------------------------------------------------------------------------
# the linear callbacks, every route, every state, every input family
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("state", GPU_STATES)
@pytest.mark.parametrize("dims", SMALL + LARGE, ids=ids)
def test_stokes_linear_callbacks(dims, state, fam):
    """Default options: each shape on the route the module docstring lists (test_route_rules)."""
    family(get_op(dims, state), dims, state, fam, with_cm=dims in CM_SHAPES and fam == "noise")


@pytest.mark.parametrize("fam", ("noise", "constant-pressure", "impulses"))
@pytest.mark.parametrize("state", ("eta", "full"))
def test_stokes_fused_z_with_pressure_sweeps(state, fam):
    """(120, 120, 68) with stokes_pressure_sweeps = 1 (read per call): the fused z launch with the pressure-gradient sweeps as
    jobs of its first launch and grad p added in the scatter, instead of the pressure folded into the stress."""
    dims = (120, 120, 68)
    with option(stokes_pressure_sweeps=1):
        family(get_op(dims, state), dims, state, fam)


@pytest.mark.parametrize("fam", ("noise", "constant-pressure"))
@pytest.mark.parametrize("state", ("default", "eta", "full"))
def test_stokes_result_vector_at_an_8_byte_offset(state, fam):
    """(120, 120, 68) with a result vector 8 bytes past a 16-byte boundary: st_fold_pressure and st_out_pairs refuse, the
    pressure-gradient sweeps and the 8-byte scatter run."""
    dims = (120, 120, 68)
    family(get_op(dims, state), dims, state, fam, offset8=True)


# ----------------------------------------------------------------------------------------------
# StokesFunction, the state it leaves, and the Jacobian apply linearised about it
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rheology", [LINEAR, POWER], ids=["linear", "power"])
@pytest.mark.parametrize("dims", SMALL + LARGE, ids=ids)
def test_stokes_function(dims, rheology):
    d = len(dims)
    N, I, g, ndv = cb.sizes(dims)
    rng = np.random.default_rng(31)
    x, dirichlet, force, xm = rng.standard_normal(g), rng.standard_normal(ndv), rng.standard_normal(g), rng.standard_normal(g)
    power = rheology[0] == 1
    variants = [("", {}, False)]
    if dims == (120, 120, 68):
        variants += [("/sweeps", {"stokes_pressure_sweeps": 1}, False), ("/offset8", {}, True)]
    op = sp.StokesOp(dims)
    try:
        op.set_rheology(*rheology)
        op.set_dirichlet(dirichlet)
        op.set_force(force)
        r = orc.stokes_function_truth(dims, x, dirichlet, force, rheology, nthreads=NT)
        for tag, opts, off8 in variants:
            with option(**opts):
                y = run(op.function, x, g, off8)
                hold(dims, y, r["y"], r["W"], "function" + tag, fn=True, power=power)
                state = [op.get_state(w) for w in range(2 + d)]
                for j in range(d):
                    c = cb.cap_strain(dims)
                    record("strain[%d]%s" % (j, tag), *lw.check(state[2 + j], r["strain"][j], r["wstrain"][j], c, "strain[%d]" % j), c)
                if power:
                    be, bde = cb.eta_bounds(dims, rheology, r)
                    record("eta" + tag, *cb.check_relative(state[0], r["eta"], be, "eta"), 1)
                    record("deta" + tag, *cb.check_relative(state[1], r["deta"], bde, "eta'"), 1)
                else:
                    assert np.all(state[0] == 1.0) and np.all(state[1] == 0.0)
                # the Jacobian apply about the state the DEVICE holds (its own eta, eta', strain are the operator's data)
                t, W = orc.stokes_truth(dims, xm, state[0], state[1], np.stack(state[2:]), nthreads=NT)
                hold(dims, run(op.mult, xm, g, off8), t, W, "linearised-mult" + tag)
    finally:
        op.destroy()


def test_device_pow_ulps():
    """The one measured number of the bar: the device's double pow against powl on the q = eps + gamma / gamma0 values of the
    power-law cases (torch.pow with a generic exponent calls the same device-library pow as the node kernels).  The allowance
    POW_ULPS must be at least twice the worst error, rounded up."""
    worst = 0.0
    for dims in SMALL + [(66, 96, 66)]:
        N, I, g, ndv = cb.sizes(dims)
        d = len(dims)
        rng = np.random.default_rng(31)
        x, dirichlet, force = rng.standard_normal(g), rng.standard_normal(ndv), rng.standard_normal(g)
        r = orc.stokes_function_truth(dims, x, dirichlet, force, POWER, nthreads=NT)
        s = r["strain"].reshape(d, -1, d)
        q = POWER[3] + 0.5 * (s * s).sum(axis=(0, 2)) / POWER[4]
        for pw in ((1.0 - POWER[2]) / (2.0 * POWER[2]), 2.5, 1.5):
            got = torch.pow(dev(q), pw).cpu().numpy()
            ref = np.power(q.astype(np.longdouble), np.longdouble(pw))
            ulps = float((np.abs(got.astype(np.longdouble) - ref) / np.spacing(np.abs(ref).astype(np.float64))).max())
            worst = max(worst, ulps)
    record("pow-ulps", worst, "-", cb.POW_ULPS)
    assert math.ceil(2 * worst) <= cb.POW_ULPS


# ----------------------------------------------------------------------------------------------
# dependence: what a call may read; recovery: what it may leave behind
# ----------------------------------------------------------------------------------------------
DEP_SHAPES = [(14, 12, 10), (120, 120, 68), (98, 96, 130)]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("state", GPU_STATES)
@pytest.mark.parametrize("dims", DEP_SHAPES, ids=ids)
def test_stokes_mult_reads_only_what_the_operator_depends_on(dims, state):
    """NaN, then +Inf, in one velocity component (then in the pressure) at the interior node (i0, j0, k0), on z-line
    i0 P1 + j0 of the last tiles and four or more nodes from every face (where the line count is no multiple of the tile, in the
    last, partial tile of interior lines).  The exact operator reads a velocity only along two successive lines: every row at
    the nodes with i != i0, j != j0 and k != k0 must keep the bits of the run with 1.0 there -- on the uniform route too
    (D_j D_j v and grad div v).  A pressure reaches the velocity rows on the three lines through its node only, and no
    pressure row.  Last, the clean vector on the handle that saw the NaN and Inf runs gives the bits of a fresh handle."""
    d = len(dims)
    node = (dims[0] - 5, dims[1] - 6, dims[2] // 2 + 1)
    op = get_op(dims, state)
    x = cb.noise(dims, 41).reshape(idims(dims) + (d + 1,))
    inode = tuple(i - 1 for i in node)
    I = np.indices(idims(dims))
    same = [I[k] == inode[k] for k in range(d)]
    far_v = ~(same[0] | same[1] | same[2])                                       # shares no index with the node
    off_lines = (same[0].astype(int) + same[1].astype(int) + same[2].astype(int)) < 2
    for comp, mask_v, mask_p in ((1, far_v, far_v), (d, off_lines, np.ones_like(far_v))):
        x[inode + (comp,)] = 1.0
        base = run(op.mult, x.reshape(-1), op.global_size).reshape(idims(dims) + (d + 1,))
        assert np.isfinite(base).all()
        for bad in (float("nan"), float("inf")):
            x[inode + (comp,)] = bad
            y = run(op.mult, x.reshape(-1), op.global_size).reshape(idims(dims) + (d + 1,))
            for k in range(d):
                assert np.array_equal(bits(y[..., k])[mask_v], bits(base[..., k])[mask_v]), (comp, bad, k)
            assert np.array_equal(bits(y[..., d])[mask_p], bits(base[..., d])[mask_p]), (comp, bad)
            assert not np.isfinite(y).all()                                      # (the bad value did arrive)
        x[inode + (comp,)] = 1.0
        again = run(op.mult, x.reshape(-1), op.global_size).reshape(idims(dims) + (d + 1,))
        assert np.array_equal(bits(again), bits(base)), comp
    fresh = make_op(dims, state)
    try:
        assert np.array_equal(bits(run(fresh.mult, x.reshape(-1), fresh.global_size)), bits(again.reshape(-1)))
    finally:
        fresh.destroy()


def idims(dims):
    return cb.idims(dims)


@pytest.mark.parametrize("rheology", [LINEAR, POWER], ids=["linear", "power"])
@pytest.mark.parametrize("dims", DEP_SHAPES, ids=ids)
def test_stokes_recovers_from_a_nan_iterate(dims, rheology):
    """A Newton line search that backtracks from a NaN iterate: function, then mult, with a vector that holds NaN (one velocity
    and one pressure entry), then the same two calls with a clean vector, on one handle.  The clean results and the state
    equal, bit for bit, those of a handle that never saw the NaN: no work array (xL, V, strain, T, pL, gp, yLx) and no flag
    (deta_nonzero, strain_stale, eta_uniform) carries anything over."""
    d = len(dims)
    N, I, g, ndv = cb.sizes(dims)
    rng = np.random.default_rng(51)
    x, dirichlet, force, xm = rng.standard_normal(g), rng.standard_normal(ndv), rng.standard_normal(g), rng.standard_normal(g)
    bad = x.copy().reshape(-1, d + 1)
    bad[I // 2, 0] = float("nan")
    bad[I // 3, d] = float("nan")
    res = []
    for poisoned in (True, False):
        op = sp.StokesOp(dims)
        try:
            op.set_rheology(*rheology)
            op.set_dirichlet(dirichlet)
            op.set_force(force)
            if poisoned:
                yb = run(op.function, bad.reshape(-1), g)
                ymb = run(op.mult, bad.reshape(-1), g)
                assert np.isnan(yb).any() and np.isnan(ymb).any()
            y = run(op.function, x, g)
            ym = run(op.mult, xm, g)
            res.append([y, ym] + [op.get_state(w) for w in range(2 + d)])
        finally:
            op.destroy()
    for k, (a, b) in enumerate(zip(*res)):
        assert np.isfinite(a).all() and np.array_equal(bits(a), bits(b)), k


# ----------------------------------------------------------------------------------------------
# EllipticOp: the Jacobian apply and FormFunction with a variable coefficient
# ----------------------------------------------------------------------------------------------
def ell_inputs(dims):
    N, G, Dn = orc.sizes(dims)
    d = len(dims)
    rng = np.random.default_rng(61)
    return dict(U=rng.standard_normal(G), Us=rng.standard_normal(G) * 10.0 ** rng.integers(-30, 31, size=G),
                eta=np.exp(rng.uniform(np.log(0.5), np.log(10.0), N)), deta=rng.standard_normal(N), g0=rng.standard_normal((d, N)),
                Uf=rng.standard_normal(G), b=rng.standard_normal(G), dv=rng.standard_normal(Dn))


def ell_truths(dims):
    if ("ell", dims) not in _TRUTH:
        a = ell_inputs(dims)
        _TRUTH[("ell", dims)] = (a, orc.elliptic_truth(dims, a["U"], a["eta"], a["deta"], a["g0"], nthreads=NT),
                                 orc.elliptic_truth(dims, a["Us"], a["eta"], a["deta"], a["g0"], nthreads=NT),
                                 orc.elliptic_function_truth(dims, a["Uf"], a["b"], a["dv"], gamma=1.0, exponent=2.0, nthreads=NT),
                                 orc.elliptic_function_truth(dims, a["Uf"], a["b"], None, gamma=1.0, exponent=2.0, nthreads=NT))
    return _TRUTH[("ell", dims)]


def run_ell(op, U, b, n, gamma=None, exponent=2.0, offset8=False):
    def at(v):
        if not offset8:
            return dev(v)
        buf = torch.empty(n + 1, dtype=torch.float64, device="cuda")
        buf[1:] = torch.from_numpy(np.ascontiguousarray(v))
        assert buf[1:].data_ptr() % 16 == 8
        return buf[1:]
    out = torch.full((n + 1,), float("nan"), dtype=torch.float64, device="cuda")
    y = out[1:] if offset8 else out[:n]
    if gamma is None:
        op.mult(at(U), y)
    else:
        op.function(at(U), None if b is None else dev(b), y, gamma, exponent)
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("opt", ELL_OPTIONS, ids=lambda o: o or "default")
@pytest.mark.parametrize("dims", ELL_SHAPES, ids=ids)
def test_elliptic_callbacks(dims, opt):
    """EllipticOp.mult after set_state of eta, eta' and grad u0, and FormFunction with gamma = 1, exponent 2, b and Dirichlet
    values, at the shapes of test_elliptic_nonlinear_* that select different kernels (short lines; odd extents; KS = 16 and 32;
    the straight-line kernel of fused4.hip at even extents of 66 .. 256 points), by default and with each option that changes
    the route (set before the handle is created); then mult about the state the device holds."""
    d = len(dims)
    a, (t, W), (ts, Ws), r, r0 = ell_truths(dims)
    with option(**({opt: 1} if opt else {})):
        op = sp.EllipticOp(dims)
        try:
            G = op.global_size
            op.set_state(0, a["eta"])
            op.set_state(1, a["deta"])
            for k in range(d):
                op.set_state(2 + k, a["g0"][k])
            c = cb.cap_e(dims)
            record("noise:mult", *lw.check(run_ell(op, a["U"], None, G), t, W, c, "mult"), c)
            record("node-scaled:mult", *lw.check(run_ell(op, a["Us"], None, G), ts, Ws, c, "mult scaled"), c)
            cf = cb.cap_e(dims, True)
            # homogeneous Dirichlet rows first (at even extents of 66 .. 256 points the interior-line launches, which leave eta and
            # eta' to be formed from w0 by whoever reads them), and the Jacobian apply about that state
            record("function-homogeneous", *lw.check(run_ell(op, a["Uf"], a["b"], G, gamma=1.0), r0["rhs"], r0["W"], cf, "function"), cf)
            ym = run_ell(op, a["U"], None, G)
            st0 = [op.get_state(w) for w in range(2 + d)]
            tm, Wm = orc.elliptic_truth(dims, a["U"], st0[0], st0[1], np.stack(st0[2:]), nthreads=NT)
            record("linearised-mult-homogeneous", *lw.check(ym, tm, Wm, c, "linearised mult"), c)
            op.set_dirichlet(a["dv"])
            record("function", *lw.check(run_ell(op, a["Uf"], a["b"], G, gamma=1.0), r["rhs"], r["W"], cf, "function"), cf)
            state = [op.get_state(w) for w in range(2 + d)]
            record("eta", *cb.check_relative(state[0], r["eta"], 3, "eta"), 1)
            record("deta", *cb.check_relative(state[1], r["deta"], 2, "eta'"), 1)
            for k in range(d):
                cg = max(dims) + 8
                record("gradu[%d]" % k, *lw.check(state[2 + k], r["gradu"][k], r["wgrad"][k], cg, "gradu[%d]" % k), cg)
            tm, Wm = orc.elliptic_truth(dims, a["U"], state[0], state[1], np.stack(state[2:]), nthreads=NT)
            record("linearised-mult", *lw.check(run_ell(op, a["U"], None, G), tm, Wm, c, "linearised mult"), c)
        finally:
            op.destroy()


def test_elliptic_callbacks_with_vectors_at_an_8_byte_offset():
    """Input and result vectors 8 bytes past a 16-byte boundary: the 8-byte-aligned fallbacks."""
    dims = (68, 70, 72)
    d = len(dims)
    a, (t, W), _, r, _ = ell_truths(dims)
    op = sp.EllipticOp(dims)
    try:
        G = op.global_size
        op.set_state(0, a["eta"])
        op.set_state(1, a["deta"])
        for k in range(d):
            op.set_state(2 + k, a["g0"][k])
        c, cf = cb.cap_e(dims), cb.cap_e(dims, True)
        record("noise:mult", *lw.check(run_ell(op, a["U"], None, G, offset8=True), t, W, c, "mult"), c)
        op.set_dirichlet(a["dv"])
        record("function", *lw.check(run_ell(op, a["Uf"], a["b"], G, gamma=1.0, offset8=True), r["rhs"], r["W"], cf, "function"), cf)
    finally:
        op.destroy()


def test_elliptic_function_with_a_real_exponent():
    """eta = 1 + gamma u^2.5 on a positive state: the device pow, with its allowance."""
    dims = (33, 40)
    N, G, Dn = orc.sizes(dims)
    rng = np.random.default_rng(62)
    U, b, dv = rng.random(G) + 0.5, rng.standard_normal(G), rng.random(Dn) + 0.5
    r = orc.elliptic_function_truth(dims, U, b, dv, gamma=1.5, exponent=2.5, nthreads=NT)
    op = sp.EllipticOp(dims)
    try:
        op.set_dirichlet(dv)
        cf = cb.cap_e(dims, True, True)
        record("function", *lw.check(run_ell(op, U, b, G, gamma=1.5, exponent=2.5), r["rhs"], r["W"], cf, "function"), cf)
        record("eta", *cb.check_relative(op.get_state(0), r["eta"], 3 + cb.POW_ULPS, "eta"), 1)
        record("deta", *cb.check_relative(op.get_state(1), r["deta"], 3 + cb.POW_ULPS, "eta'"), 1)
    finally:
        op.destroy()


@pytest.mark.parametrize("dims", [(12, 11, 10), (68, 70, 72), (132, 68, 130)], ids=ids)
def test_elliptic_recovers_from_a_nan_iterate(dims):
    """function, then mult, with a NaN in the vector; then the clean vector: the bits of a handle that never saw the NaN."""
    a = ell_inputs(dims)
    d = len(dims)
    bad = a["Uf"].copy()
    bad[bad.size // 2] = float("nan")
    res = []
    for poisoned in (True, False):
        op = sp.EllipticOp(dims)
        try:
            G = op.global_size
            op.set_dirichlet(a["dv"])
            if poisoned:
                assert np.isnan(run_ell(op, bad, a["b"], G, gamma=1.0)).any() and np.isnan(run_ell(op, bad, None, G)).any()
            y = run_ell(op, a["Uf"], a["b"], G, gamma=1.0)
            ym = run_ell(op, a["U"], None, G)
            res.append([y, ym] + [op.get_state(w) for w in range(2 + d)])
        finally:
            op.destroy()
    for k, (p, q) in enumerate(zip(*res)):
        assert np.isfinite(p).all() and np.array_equal(bits(p), bits(q)), k
