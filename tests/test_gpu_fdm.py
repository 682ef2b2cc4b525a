"""The fast-diagonalisation solve (csrc/precond.hip: fdm_solve) against a long-double truth, step by step (fdm_ref.py).

  a. every step of the solve (FdPc.step / SpectralPc.step / HelmholtzSolver.step: the very function the solve is made of), element by
     element, against the derived caps of fdm_ref.step_cap; one NaN / +Inf line leaves every other line's bits alone; step_route
     says which kernels ran;
  b. the steps run by hand in the solve's order give apply / solve bit for bit;
  c. the whole solve against the long-double chain: per stacked field max-norm and 2-norm error <= 16 x the larger error of the two
     double restatements on the same input;
  e. containment and state: NaN in one stacked field, a clean call after it, first use, in place, update();
  f. the stencil of MatVVPC with variable viscosity against the oracle's matrix, per element.

The cases of BASE_CASES name the routes they are there to reach; a route that is not reached is a failure."""
import os

import numpy as np
import pytest
import torch
import scipy.sparse as sps

import __graft_entry__ as ge
import oracle_lib as orc
import linewise as lw
import fdm_ref as fr
from conftest import relerr

pytestmark = pytest.mark.gpu
sp = ge.load()
LD = np.longdouble
SEED = 20241019
MARGIN = 16.0
SMALL = 60000                     # values above which the generator inputs are checked on fdm_ref.sample_lines, not on every line
RATIOS = {}                       # (kind, route) -> worst ratio; written out when the module is done where FDM_RATIOS_OUT names a file


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    """Where FDM_RATIOS_OUT names a file: the worst ratios the tests of this module that ran have measured, per step and route
    (profiles/fdm/ratios.txt)."""
    yield
    path = os.environ.get("FDM_RATIOS_OUT")
    if path and RATIOS:
        with open(path, "w") as f:
            for (kind, route), v in sorted(RATIOS.items()):
                f.write("%-40s %-70s %.3f\n" % (kind, route, v))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def nan_like(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def log_eta(dims, seed):
    return np.exp(np.random.default_rng(seed).uniform(np.log(0.5), np.log(10.0), int(np.prod(dims))))


# ----------------------------------------------------------------------------------------------
# handles
# ----------------------------------------------------------------------------------------------
class Case:
    """One handle with what the reference needs to restate its solve: lines L, sigma, the interior viscosity (None: no division),
    nf stacked fields, and `solve` on component-major arrays."""

    def __init__(self, spec, dims, seed=SEED):
        self.spec, self.dims, self.d = spec, tuple(dims), len(dims)
        self.inner = tuple(p - 2 for p in dims)
        self.G = int(np.prod(self.inner))
        self.sigma, self.eta, self.bc, self.scale = 0.0, None, None, None
        self.node_major = False
        self.op = None
        name = spec[0]
        if name in ("ell", "spec"):
            self.op = op = sp.EllipticOp(dims)
            if spec[1] == "var":                       # eta = 1 + u^2 of a FormFunction (gamma = 1)
                u = dev(np.random.default_rng(seed + 3).uniform(0.0, 2.0, op.global_size))
                op.function(u, dev(np.zeros(op.global_size)), nan_like(op.global_size), 1.0, 2.0)
                torch.cuda.synchronize()
            if name == "spec":
                self.sigma = 1.5
                self.h = sp.SpectralPc(op, self.sigma)
            else:
                self.h = sp.FdPc(op, sweeps=0)
            self.kind, self.nf = ("spectral" if name == "spec" else "fd"), 1
            self.call = self.h.apply
        elif name == "stokes":
            self.op = op = sp.StokesOp(dims)
            if spec[1] == "var":
                op.set_state(0, log_eta(dims, seed + 4))
            self.h = sp.FdPc(op, sweeps=0)
            self.kind, self.nf = "fd", self.d
            self.node_major = spec[2] == "nm"
            self.call = self.h.apply if self.node_major else self.h.apply_cm
        else:                                          # ("helm", sigma, nfields[, bc[, scale]])
            self.sigma, self.nf = float(spec[1]), int(spec[2])
            self.bc = spec[3] if len(spec) > 3 else None
            self.scale = spec[4] if len(spec) > 4 else None
            self.h = sp.HelmholtzSolver(dims, self.sigma, self.nf, bc=self.bc, scale=self.scale)
            self.kind = "spectral"
            self.call = self.h.solve
        self.over_eta = self.op is not None
        self.n = self.nf * self.G
        self.shape = (self.nf,) + self.inner
        self.L = fr.lines(sp, self.kind, dims, bc=self.bc, scale=self.scale)
        self.parity = [True] * self.d if self.bc is None else [fr.parity_ok(b) for b in self.bc]
        self.refresh_eta()

    def refresh_eta(self):
        """The interior viscosity from the operator's own state, by slicing: nothing the preconditioner computed."""
        if self.op is not None:
            self.eta = fr.interior(self.op.get_state(0), self.dims)

    def to_abi(self, x):
        """component-major (nf, ...) NumPy array -> the flat array of the handle's solve"""
        x = np.asarray(x).reshape(self.nf, self.G)
        return np.ascontiguousarray(x.T).ravel() if self.node_major else x.ravel()

    def from_abi(self, z):
        z = np.asarray(z)
        return np.ascontiguousarray(z.reshape(self.G, self.nf).T).reshape(self.shape) if self.node_major else z.reshape(self.shape)

    def solve(self, x, offset8=False):
        """The handle's own solve of the component-major NumPy array x; offset8: on vectors that are only 8-byte aligned."""
        a = self.to_abi(x)
        if offset8:
            bx = torch.empty(self.n + 1, dtype=torch.float64, device="cuda")
            bz = torch.full((self.n + 1,), float("nan"), dtype=torch.float64, device="cuda")
            xi, zo = bx[1:], bz[1:]
            assert xi.data_ptr() % 16 == 8 and zo.data_ptr() % 16 == 8
            xi.copy_(torch.from_numpy(a))
        else:
            xi, zo = dev(a), nan_like(self.n)
        self.call(xi, zo)
        return self.from_abi(host(zo))

    def plan(self):
        """The solve's steps [(mode, k)], found by asking step_route which modes the handle takes -- a refused mode is never run."""
        d, h = self.d, self.h
        first = "forward_over_eta" if self.over_eta and not self.node_major else "forward"
        steps = []
        z = h.step_route(d - 1, "zsolve") is not None
        for k in range(d):
            if k == d - 1 and d >= 2:
                if z:
                    steps.append(("zsolve", k))
                    continue
                if h.step_route(k, "forward_scaled") is not None:
                    steps.append(("forward_scaled", k))
                    continue
            steps.append((first if k == 0 else "forward", k))
            assert h.step_route(k, steps[-1][0]) is not None, steps[-1]
        if steps[-1][0] in ("forward", "forward_over_eta"):
            steps.append(("scale", d - 1))
        for k in range(d - 2 if z else d - 1, -1, -1):
            steps.append(("backward", k))
        return steps

    def run_step(self, mode, k, x):
        """One step on a component-major NumPy array; returns the NumPy result."""
        xi = dev(np.asarray(x).ravel())
        return host(self.h.step(k, mode, xi, nan_like(self.n))).reshape(self.shape)

    def by_hand(self, x, offset8=False):
        """The solve composed from its steps: [(mode, k, input, output)] as NumPy arrays, the device buffers chained as they are.
        offset8: the first step reads and the last one writes an array that is only 8-byte aligned, as the solve does on such vectors."""
        cur = dev(np.asarray(x).ravel())
        if self.node_major:                            # (chebhip_fdpc_apply divides while it pulls the components apart)
            cur = (cur.reshape(self.nf, self.G) / dev(self.eta.ravel())[None, :]).reshape(-1).contiguous()
        if offset8:
            buf = torch.empty(self.n + 1, dtype=torch.float64, device="cuda")
            buf[1:].copy_(cur)
            cur = buf[1:]
            assert cur.data_ptr() % 16 == 8
        out = []
        plan = self.plan()
        for q, (mode, k) in enumerate(plan):
            dst = nan_like(self.n + 1)[1:] if offset8 and q == len(plan) - 1 else nan_like(self.n)
            nxt = self.h.step(k, mode, cur, dst)
            out.append((mode, k, host(cur).reshape(self.shape).copy(), host(nxt).reshape(self.shape).copy()))
            cur = nxt
        return out

    def eta_for(self, mode):
        return self.eta

    def destroy(self):
        self.h.destroy()
        if self.op is not None:
            self.op.destroy()


def route_name(r):
    return "+".join(sorted(r)) if r else "none"


def record(kind, route, ratio):
    key = (kind, route)
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(ratio))


def check_step(c, mode, k, x, y, tag, lines=None):
    """The bar of one step (lines: on these lines of direction k only, fdm_ref.sample_lines; the step itself ran on all of them): |y_i - truth_i| <= cap 2^-53 B_i (fdm_ref.step_cap, linewise.bound), B_i = 0 demanding an exact 0, on
    every route.  Below the normal range a result is rounded to a multiple of 2^-1074 instead (some entries of S^-1 of a 256-point
    line are that small): one such unit per counted rounding is allowed on top, B_i + 2^-1021 where B_i > 0.
    (The two-launch form of the backward transform stays inside B_i: the columns of S are the parity modes, so |S_m-i,m-j| =
    |S_i,m-j| and both parts (S +- J S J) / 2 are bounded by the symmetrised row (|S_ij| + |S_i,m-j|) / 2 that B_i is built on.
    The same form of S^-1, whose ROWS are the modes, mixed rows i and m - i and missed B_i by factors up to 8e3: the forward
    transform is a dense product with S^-1 itself wherever it is not one raw launch.)"""
    t, B = fr.step_truth_bound(mode, k, x, c.L, c.sigma, c.eta, lines=lines)
    if lines is not None:
        y = lw.take_lines(y, k + 1, lines)
    cap = fr.step_cap(mode, c.inner[k], c.d)
    route = c.h.step_route(k, mode)
    B = np.where(B > 0, B + 2.0 ** -1021, 0.0)
    r, _ = lw.check(y, t, B, cap, what="%s %s[%d] %s" % (tag, mode, k, route_name(route)))
    record("step %s (fraction of cap)" % mode, route_name(route), r / cap)
    return r / cap


def poisoned_lines(c, k, tile=32):
    """The lines of direction k (flat index over the stacked fields and the other directions) that get a NaN or +Inf: the first and
    the last line, both sides of the boundary between stacked fields 0 and 1 (inside one tile of the z solve where the lines per field
    are no multiple of the tile), the first line of the last, partial tile, and one in the middle."""
    nl = c.n // c.inner[k]
    per = nl // c.nf
    sel = [0, nl - 1, nl // 3, ((nl - 1) // tile) * tile]
    if c.nf > 1:
        sel += [per - 1, per]
    return sorted(set(sel))


def check_lines_contained(c, mode, k, x, y, tag):
    """One line with a NaN or +Inf (in turn) in one element: every other line of the step's output keeps its bits, on all lines."""
    K = c.inner[k]
    xm = np.moveaxis(np.array(x), k + 1, -1).reshape(-1, K)
    ym = np.moveaxis(y, k + 1, -1).reshape(-1, K)
    nl = xm.shape[0]
    for q, line in enumerate(poisoned_lines(c, k)):
        bad = (np.nan, np.inf)[q & 1]
        xb = xm.copy()
        xb[line, (K // 2, 0, K - 1)[q % 3]] = bad
        xb = np.moveaxis(xb.reshape([c.shape[j] for j in range(c.d + 1) if j != k + 1] + [K]), -1, k + 1)
        yb = np.moveaxis(c.run_step(mode, k, np.ascontiguousarray(xb)), k + 1, -1).reshape(-1, K)
        keep = np.arange(nl) != line
        assert np.array_equal(yb[keep], ym[keep]), "%s %s[%d]: a %r in line %d changed another line" % (tag, mode, k, bad, line)
        assert not np.all(np.isfinite(yb[line]))


def check_composite(c, x, z, tag, route):
    """(c): per stacked field both error measures <= MARGIN x the larger restatement error on this input."""
    t = fr.truth(x, c.L, c.sigma, c.eta)
    e_dev = fr.errors(z, t)
    e_ref = [fr.errors(fr.chain(x, c.L, c.sigma, c.eta, how, parity=c.parity)[0], t) for how in ("plain", "evenodd")]
    worst = 0.0
    for f in range(c.nf):
        for q, what in enumerate(("max", "l2")):
            ref = max(e[f][q] for e in e_ref)
            ratio = e_dev[f][q] / ref if ref > 0 else (0.0 if e_dev[f][q] == 0 else np.inf)
            worst = max(worst, ratio)
            print("    %s field %d %s: device %.3g, restatements %.3g / %.3g, ratio %.2f" % (tag, f, what, e_dev[f][q], e_ref[0][f][q], e_ref[1][f][q], ratio))
            assert ratio <= MARGIN, "%s field %d %s-error %.3g = %.1f x the restatements' %.3g (bar %g)" % (tag, f, what, e_dev[f][q], ratio, ref, MARGIN)
    record("solve (device / restatement)", route, worst)


# ----------------------------------------------------------------------------------------------
# the cases: shape, handle, option, what the case is there to reach
# ----------------------------------------------------------------------------------------------
ELL1, ELLV, SPECV = ("ell", "unit"), ("ell", "var"), ("spec", "var")
ST1C, STVC, ST1N, STVN = ("stokes", "unit", "cm"), ("stokes", "var", "cm"), ("stokes", "unit", "nm"), ("stokes", "var", "nm")
H1, H3, H1K = ("helm", 0.0, 1), ("helm", 1.5, 3), ("helm", 1e3, 1)
NEU2, NEU3 = ("helm", 0.0, 1, ("neumann", "neumann")), ("helm", 0.0, 1, ("neumann", "neumann", "neumann"))
ROBIN = ("helm", 0.5, 3, ((1.0, 0.5), (2.0, 1.0)))
MIXED = ("helm", 0.0, 1, ("dirichlet", ("dirichlet", "neumann")))
BOX = ("helm", 1.5, 3, ("neumann", "dirichlet", (1.0, 1.0)), (0.5, 1.0, 2.0))

# expectation: {(mode, k): set of route names that must ALL be present} ("absent": the mode must be refused)
R, F, T2, GEN, Z, S3, SG, EP, DN = "raw", "fused_mul", "two_launch", "general", "zsolve", "scale3", "scale_general", "eta_pass", "dense"
CASES = [
    # stride 8: no raw launch in direction 0 (forward: the dense product; backward: two launches)
    ((9,), ELLV, None, {("forward_over_eta", 0): {EP}, ("scale", 0): {S3}}),
    ((9,), H1, None, {("scale", 0): {S3}}),
    ((12, 10), ELLV, None, {("forward_over_eta", 0): {DN, EP}, ("backward", 0): {T2}}),
    ((12, 10), STVC, None, {("forward_over_eta", 0): {DN, EP}, ("backward", 0): {T2}}),
    ((12, 10), H3, None, {("forward", 0): {DN}, ("backward", 0): {T2}}),
    # odd lines
    ((8, 7, 6), ELLV, None, {("forward_over_eta", 0): {EP}}),
    ((8, 7, 6), STVN, None, {}),
    ((8, 7, 6), SPECV, None, {("forward_over_eta", 0): {EP}}),
    # raw strided and raw contiguous, short lines
    ((20, 18, 18), ELL1, None, {("forward_over_eta", 0): {R, EP}, ("forward", 1): {R}, ("forward_scaled", 2): {R, F}, ("backward", 0): {R}}),
    ((20, 18, 18), STVC, None, {("forward_over_eta", 0): {R, EP}, ("forward_scaled", 2): {R, F}}),
    ((20, 18, 18), STVN, None, {("forward", 0): {R}, ("forward_scaled", 2): {R, F}}),
    ((20, 18, 18), H3, None, {("forward", 0): {R}, ("forward_scaled", 2): {R, F}}),
    ((66, 12, 5), ELLV, None, {}),
    ((66, 12, 5), H1K, None, {}),
    # load-side eta at 128 points, z solve at 68
    ((130, 70), ELLV, None, {("forward_over_eta", 0): {R, F}, ("zsolve", 1): {Z}}),
    ((130, 70), STVC, None, {("forward_over_eta", 0): {R, F}, ("zsolve", 1): {Z}}),
    ((130, 70), SPECV, None, {("forward_over_eta", 0): {R, F}, ("zsolve", 1): {Z}}),
    ((130, 70), H1, None, {("forward", 0): {R}, ("zsolve", 1): {Z}}),
    # odd long lines, first and last
    ((131, 70), ELLV, None, {("zsolve", 1): {Z}}),
    ((70, 131), ELLV, None, {("zsolve", 1): "absent"}),
    ((70, 131), H3, None, {("zsolve", 1): "absent"}),
    # KS = 32 with load-side eta; store-side scaling at 18
    ((258, 20), ELLV, None, {("forward_over_eta", 0): {R, F}, ("forward_scaled", 1): {R, F}}),
    ((258, 20), SPECV, None, {("forward_over_eta", 0): {R, F}, ("forward_scaled", 1): {R, F}}),
    # z solve, H = 64 / 63 / 33 with tiles that straddle fields
    ((20, 18, 130), STVC, None, {("zsolve", 2): {Z}}),
    ((20, 18, 130), STVN, None, {("zsolve", 2): {Z}}),
    ((20, 18, 130), H3, None, {("zsolve", 2): {Z}}),
    ((20, 18, 128), STVC, None, {("zsolve", 2): {Z}}),
    ((20, 18, 128), ELL1, None, {("zsolve", 2): {Z}}),
    ((36, 70, 68), STVC, None, {("zsolve", 2): {Z}}),
    ((36, 70, 68), H1, None, {("zsolve", 2): {Z}}),
    # 256-point last line: store-side scaling, no z solve
    ((12, 10, 258), ELLV, None, {("zsolve", 2): "absent", ("forward_scaled", 2): {R, F}}),
    ((12, 10, 258), H3, None, {("zsolve", 2): "absent", ("forward_scaled", 2): {R, F}}),
    # 65 536 lines: the general scaling kernel at d = 3
    ((258, 258, 5), ELLV, None, {("scale", 2): {SG}}),
    ((258, 258, 5), H1, None, {("scale", 2): {SG}}),
    # d >= 4
    ((5, 4, 4, 3), ELLV, None, {("scale", 3): {SG}}),
    ((5, 4, 4, 3), H3, None, {("scale", 3): {SG}}),
    ((6,) * 5, ELLV, None, {("scale", 4): {SG}}),
    ((6,) * 5, H1, None, {("scale", 4): {SG}}),
    # option routes
    ((130, 70), ELLV, "fdm_passes", {("forward_over_eta", 0): {R, EP}, ("zsolve", 1): "absent", ("scale", 1): {S3}}),
    ((20, 18, 130), STVC, "fdm_passes", {("forward_over_eta", 0): {EP}, ("zsolve", 2): "absent", ("scale", 2): {S3}}),
    ((20, 18, 18), H3, "fdm_passes", {("forward_scaled", 2): "absent", ("scale", 2): {S3}}),
    ((130, 70), ELLV, "fdm_z_separate", {("zsolve", 1): "absent", ("forward_scaled", 1): {R, F}, ("backward", 1): {R}}),
    ((20, 18, 130), STVC, "fdm_z_separate", {("zsolve", 2): "absent", ("forward_scaled", 2): {R, F}}),
    ((36, 70, 68), H1, "fdm_z_separate", {("zsolve", 2): "absent", ("forward_scaled", 2): {R, F}}),
    ((130, 70), ELLV, "no_raw_transforms", {("forward_over_eta", 0): {DN, EP}, ("zsolve", 1): "absent", ("scale", 1): {S3}, ("backward", 0): {T2}}),
    ((20, 18, 130), STVC, "no_raw_transforms", {("forward_over_eta", 0): {DN, EP}, ("zsolve", 2): "absent", ("backward", 2): {T2}}),
    ((20, 18, 18), H3, "no_raw_transforms", {("forward", 0): {DN}, ("scale", 2): {S3}, ("backward", 0): {T2}}),
    ((130, 70), ELLV, "general_kernels", {("forward_over_eta", 0): {DN, EP}, ("zsolve", 1): "absent", ("backward", 1): {T2, GEN}}),
    ((20, 18, 130), STVC, "general_kernels", {("forward_over_eta", 0): {DN, EP}, ("zsolve", 2): "absent", ("backward", 2): {T2, GEN}}),
    ((20, 18, 18), H3, "general_kernels", {("forward", 0): {DN}, ("scale", 2): {S3}, ("backward", 0): {T2, GEN}}),
    # vectors at an 8-byte offset (the solve's first and last transform see them)
    ((130, 70), ELLV, "offset8", {("zsolve", 1): {Z}}),
    ((20, 18, 130), H3, "offset8", {("zsolve", 2): {Z}}),
    ((12, 10), STVC, "offset8", {}),
    # boundary-condition handles
    ((20, 70), NEU2, None, {("zsolve", 1): {Z}}),
    ((12, 10, 70), NEU3, None, {("zsolve", 2): {Z}}),
    ((20, 70), ROBIN, None, {("zsolve", 1): {Z}}),
    ((20, 70), MIXED, None, {("zsolve", 1): "absent", ("forward", 1): {DN}, ("backward", 1): {T2}}),
    ((20, 18, 18), BOX, None, {}),
]


# ... and the rest of the table: every shape on every kind of handle by default, and under every option on the kind OPTION_HANDLE names; these
# cases name no route of their own (the steps, the composition and the solve are held as everywhere)
SHAPES = [(9,), (12, 10), (8, 7, 6), (20, 18, 18), (66, 12, 5), (130, 70), (131, 70), (70, 131), (258, 20), (20, 18, 130), (20, 18, 128),
          (36, 70, 68), (12, 10, 258), (258, 258, 5), (5, 4, 4, 3), (6,) * 5]
HANDLES = [ELL1, ELLV, ST1C, STVC, ST1N, STVN, SPECV, H1, H3, H1K]
OPTIONS = ["fdm_passes", "fdm_z_separate", "no_raw_transforms", "general_kernels"]
BASE_CASES = list(CASES)


# the kind of handle every option runs on at each shape, written out (a StokesOp is 2-D / 3-D)
OPTION_HANDLE = {(9,): ELLV, (12, 10): STVC, (8, 7, 6): STVN, (20, 18, 18): ST1C, (66, 12, 5): H3, (130, 70): SPECV, (131, 70): H1K,
                 (70, 131): ST1N, (258, 20): H3, (20, 18, 130): ELLV, (20, 18, 128): STVN, (36, 70, 68): H3, (12, 10, 258): STVC,
                 (258, 258, 5): SPECV, (5, 4, 4, 3): H1, (6,) * 5: ELL1}


def _more_cases():
    have = {(v[0], v[1], v[2]) for v in BASE_CASES}
    # (three stacked fields of (258,258,5) cost 5 s of long-double products per case, and the route that shape is there for, the
    # general scaling kernel, is the same launch for one field and for three)
    ok = lambda dims, spec: (spec[0] != "stokes" or len(dims) in (2, 3)) and not (dims == (258, 258, 5) and (spec[0] == "stokes" or spec is H3))
    out = []
    for dims in SHAPES:
        for spec in HANDLES:
            if ok(dims, spec) and (dims, spec, None) not in have:
                out.append((dims, spec, None, {}))
    for option in OPTIONS:
        for dims in SHAPES:
            if (dims, OPTION_HANDLE[dims], option) not in have:
                out.append((dims, OPTION_HANDLE[dims], option, {}))
    return out


CASES = BASE_CASES + _more_cases()


def case_id(v):
    dims, spec, option, _ = v
    s = "-".join(str(x) if not isinstance(x, tuple) else "bc" for x in spec)
    return "%s-%s-%s" % ("x".join(map(str, dims)), s, option or "default")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_steps_composition_and_solve(case):
    dims, spec, option, expect = case
    offset8 = option == "offset8"
    if option and not offset8:
        sp.set_option(option, 1)
    try:
        c = Case(spec, dims)
        try:
            tag = case_id(case)
            plan = c.plan()
            # the routes this case is there to reach
            print("\n  %s: %s" % (tag, ", ".join("%s[%d] %s" % (m, k, route_name(c.h.step_route(k, m))) for m, k in plan)))
            for (mode, k), want in expect.items():
                got = c.h.step_route(k, mode)
                if want == "absent":
                    assert got is None and (mode, k) not in plan, "%s: %s[%d] should be refused, runs %r" % (tag, mode, k, got)
                    with pytest.raises(sp.ChebhipError):
                        c.h.step(k, mode, dev(np.zeros(c.n)), nan_like(c.n))
                else:
                    assert (mode, k) in plan and got is not None and want <= got, "%s: %s[%d] runs %r, the case wants %r" % (tag, mode, k, got, sorted(want))
            solve_route = " ".join("%s:%s" % (m, route_name(c.h.step_route(k, m))) for m, k in plan if m not in ("backward",) or k == 0)
            for name, x in (("noise", np.random.default_rng(SEED + 1).standard_normal(c.shape)), ("scaled", fr.node_scaled(c.shape, SEED + 2))):
                z = c.solve(x, offset8)
                # (a) on the solve's own intermediates, (b) bit for bit
                steps = c.by_hand(x, offset8)
                for mode, k, xi, yi in steps:
                    check_step(c, mode, k, xi, yi, "%s %s" % (tag, name))
                assert np.array_equal(steps[-1][3], z), "%s %s: the steps by hand differ from the solve" % (tag, name)
                # (step_route speaks of the handle's own aligned buffers: at an offset the first and the last step see a
                # misaligned array and take the route that does not need the alignment)
                label = "offset8 (first / last step on a misaligned array: not the route listed for it)" if offset8 else option or "default"
                check_composite(c, x, z, "%s %s" % (tag, name), "%s | %s" % (label, solve_route))
            # (a) every generator through every step, with containment of a NaN / +Inf line; the step runs on the whole array and
            # large cases compare a sample of its lines (the tiles that straddle stacked fields, the last tile, seeded ones)
            for mode, k in plan:
                lines = None if c.n <= SMALL else fr.sample_lines(c.shape, k, SEED + 12)
                for gname, gen in lw.GENERATORS.items():
                    x = gen(c.shape, k + 1, SEED + 11)
                    y = c.run_step(mode, k, x)
                    check_step(c, mode, k, x, y, "%s %s" % (tag, gname), lines=lines)
                    if gname == "noise":
                        check_lines_contained(c, mode, k, x, y, tag)
        finally:
            c.destroy()
    finally:
        if option and not offset8:
            sp.set_option(option, 0)


FALLBACK_CASES = [v for v in BASE_CASES if v[2] != "offset8" and (v[0] in ((9,), (12, 10), (8, 7, 6), (66, 12, 5), (70, 131), (258, 258, 5), (5, 4, 4, 3), (6,) * 5)
                                                                   or v[2] in ("no_raw_transforms", "general_kernels") or v[1] is MIXED)]


@pytest.mark.parametrize("case", FALLBACK_CASES, ids=case_id)
def test_fallback_transforms_meet_the_rowwise_bar(case):
    """The transforms that are not one raw launch -- forward: one dense line product with S^-1; backward: the centro-symmetric plus
    the centro-antisymmetric part of S, two launches -- against B_i on every input generator, at every shape and option that takes
    them.  This is the test that found the forward transform, then also in two parts, at 14.9 (cap 11) on noise at (66,12,5), 37 ...
    84 (11) at (258,258,5), 2.9e3 (138) on impulses at (130,70) under no_raw_transforms and 8.0e3 (76) at (70,131)."""
    dims, spec, option, _ = case
    if option:
        sp.set_option(option, 1)
    try:
        c = Case(spec, dims)
        try:
            steps = [(m, k) for m, k in c.plan() if {"two_launch", "dense"} & c.h.step_route(k, m)]
            assert steps and any("dense" in c.h.step_route(k, m) for m, k in steps), "%s: no fall-back transform" % case_id(case)
            for mode, k in steps:
                for gname, gen in lw.GENERATORS.items():
                    x = gen(c.shape, k + 1, SEED + 11)
                    check_step(c, mode, k, x, c.run_step(mode, k, x), "%s %s" % (case_id(case), gname))
        finally:
            c.destroy()
    finally:
        if option:
            sp.set_option(option, 0)


# ----------------------------------------------------------------------------------------------
# (e) containment and state
# ----------------------------------------------------------------------------------------------
STATE_CASES = [((12, 10), H3), ((20, 18, 18), H3), ((20, 18, 130), H3), ((36, 70, 68), STVC), ((20, 18, 130), STVN), ((20, 18, 18), STVC), ((130, 70), STVN)]


@pytest.mark.parametrize("dims,spec", STATE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v[0], int) else "-".join(map(str, v)))
def test_containment_and_state(dims, spec):
    """NaN (then +Inf) in one element of stacked field 1: the other fields equal the clean run bit for bit and field 1 is NaN
    throughout; a clean call after it, and the second call of a new handle, give a fresh handle's first bits; in place (solver
    handles) gives the same bits."""
    c, fresh = Case(spec, dims), None
    try:
        fresh = _containment_and_state(c, dims, spec)
    finally:
        if fresh is not None:
            fresh.destroy()
        c.destroy()


def _containment_and_state(c, dims, spec):
    x = np.random.default_rng(SEED + 21).standard_normal(c.shape)
    z_first = c.solve(x)                                    # first use: W is built in this call
    z_second = c.solve(x)
    assert np.array_equal(z_first, z_second)
    for bad in (np.nan, np.inf):
        xb = x.copy()
        xb[(1,) + tuple(s // 2 for s in c.inner)] = bad
        zb = c.solve(xb)
        for f in range(c.nf):
            if f == 1:                                      # (a NaN spreads as NaN; an Inf as Inf or NaN: nothing finite is left)
                assert np.all(np.isnan(zb[f])) if np.isnan(bad) else not np.any(np.isfinite(zb[f])), "field 1 after %r" % bad
            else:
                assert np.array_equal(zb[f], z_first[f]), "field %d changed by a %r in field 1" % (f, bad)
        assert np.array_equal(c.solve(x), z_first), "a clean call after %r differs" % bad
    fresh = Case(spec, dims)
    try:
        assert np.array_equal(fresh.solve(x), z_first)
    except BaseException:
        fresh.destroy()
        raise
    if spec[0] == "helm":
        t = dev(x.ravel())
        c.h.solve(t, t)
        assert np.array_equal(host(t).reshape(c.shape), z_first)
    return fresh


@pytest.mark.parametrize("dims,spec", [((130, 70), STVC), ((20, 18, 130), STVN), ((20, 18, 18), STVC), ((258, 20), ELLV)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v[0], int) else "-".join(map(str, v)))
def test_update_takes_the_new_viscosity(dims, spec):
    """After the viscosity changes and update() the handle equals a fresh one on the new state bit for bit (Einv rebuilt, nothing
    stale), and meets (c) with the new eta."""
    c, fresh = Case(spec, dims), None
    try:
        fresh = _update_takes_the_new_viscosity(c, dims, spec)
    finally:
        if fresh is not None:
            fresh.destroy()
        c.destroy()


def _update_takes_the_new_viscosity(c, dims, spec):
    x = np.random.default_rng(SEED + 22).standard_normal(c.shape)
    z_old = c.solve(x)
    if spec[0] == "stokes":
        c.op.set_state(0, log_eta(dims, SEED + 99))
    else:
        u = dev(np.random.default_rng(SEED + 98).uniform(0.0, 3.0, c.op.global_size))
        c.op.function(u, dev(np.zeros(c.op.global_size)), nan_like(c.op.global_size), 1.0, 2.0)
        torch.cuda.synchronize()
    c.h.update()
    c.refresh_eta()
    z_new = c.solve(x)
    assert not np.array_equal(z_new, z_old)
    fresh = sp.FdPc(c.op, sweeps=0)
    call = fresh.apply if c.node_major else (fresh.apply_cm if spec[0] == "stokes" else fresh.apply)
    z_fresh = c.from_abi(host(call(dev(c.to_abi(x)), nan_like(c.n))))
    try:
        assert np.array_equal(z_new, z_fresh)
        check_composite(c, x, z_new, "update %s" % "x".join(map(str, dims)), "after update")
    except BaseException:
        fresh.destroy()
        raise
    return fresh


# ----------------------------------------------------------------------------------------------
# (f) the stencil with variable viscosity on Stokes
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(10, 9), (7, 6, 5), (20, 18, 16)], ids=lambda d: "x".join(map(str, d)))
def test_stokes_stencil_with_variable_viscosity(dims):
    """FdPc(StokesOp).mult against kron(fd_matrix(dims, eta), I_d): normwise the 1e-13 of the eta == 1 test, and per element
    |y_i - (P x)_i| <= c 2^-53 sum_j |P_ij| |x_j| with c = 3 d + 4: 2 d + 1 products summed (a rounding each, fused or not), and a
    diagonal coefficient that the device may form with fused multiply-adds where the oracle rounds each product: d + 3 roundings of
    a sum of positive terms.  The off-diagonal coefficients are the same operations in both.  A NaN in x reaches the rows of its
    stencil, in its own component, and nothing else."""
    d = len(dims)
    st = sp.StokesOp(dims)
    eta = log_eta(dims, SEED + 31)
    st.set_state(0, eta)
    pc = sp.FdPc(st, sweeps=0)
    try:
        _stokes_stencil(dims, d, st, pc)
    finally:
        pc.destroy(); st.destroy()


def _stokes_stencil(dims, d, st, pc):
    n = st.velocity_size
    x = np.random.default_rng(SEED + 32).standard_normal(n)
    P1 = orc.fd_matrix(dims, st.get_state(0))
    P = sps.kron(P1, sps.identity(d)).tocsr()
    y = host(pc.mult(dev(x), nan_like(n)))
    assert relerr(y, P @ x) < 1e-13
    t = np.asarray(P.astype(LD) @ x.astype(LD)).ravel()
    B = np.asarray(abs(P) @ np.abs(x)).ravel()
    r, _ = lw.check(y, t, B, 3 * d + 4, what="stokes stencil %s" % (dims,))
    record("stencil (fraction of cap)", "k_fd_mult", r / (3 * d + 4))
    j = (n // (2 * d)) * d + 1                               # a node in the middle, component 1
    xb = x.copy(); xb[j] = np.nan
    yb = host(pc.mult(dev(xb), nan_like(n)))
    reach = np.zeros(n, dtype=bool)
    reach[P[:, j].nonzero()[0]] = True
    assert np.all(np.isnan(yb[reach])) and np.array_equal(yb[~reach], y[~reach])
    assert reach.sum() <= 2 * d + 1 and np.all(reach.nonzero()[0] % d == 1)
