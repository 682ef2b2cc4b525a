"""The restarted flexible GMRES (csrc/krylov.hip) against long-double truth, step by step (krylov_ref.py).

A solve is driven through Python callbacks that record (clone) every vector the solver hands out and every vector they return, and,
on the reduction path, the device's own sums: the exact bits of V_0 .. V_j, z_j = M v_j, w = A z_j, hcol and nsq of every iteration of
every cycle.  Every step then has a local truth:

  a. every step bar of krylov_ref.check_trace on every accepted iteration (first vector, stored vector, observed dots and squares, the
     norm on the three-launch step), the whole-solve bar (max-norm and 2-norm error against the long-double solve <= 16 x the larger
     error of the two double restatements; the same for the reported residual where the last column is not an estimated one), the
     iteration count and the reason -- on every case of krylov_ref.CASES: sizes 0 .. 3, the GsShared limit (restart 256), the KB row
     groups, the k % 4 tails, the second trip of gs_row_sums, the second grid-stride trip of the 8-byte and the 16-byte route; the
     one-reduction and the three-launch step; no reduction, a doubling and an identity reduction callback; no, a fixed and a varying
     preconditioner; x arriving as NaN or as a guess; the iteration limit at the end of a cycle, inside one and after several;
  b. the identity callback reproduces the solve without one;
  c. b an eigenvector: one iteration, x = b / lambda to T_dot + 6 roundings;
  d. A = 0, b = 0 and an operator that turns NaN: reason and x, and a clean solve on the same handle afterwards gives the bits of a
     fresh handle (the ticket, rn, G, the pinned residuals);
  e. the same solve twice gives the same bits, through Python callbacks and through a C entry point.

Where KRYLOV_RATIOS_OUT names a file the worst ratio per bar and route is written there (profiles/krylov/ratios.txt)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import krylov_ref as kr

pytestmark = pytest.mark.gpu
sp = ge.load()
LD = kr.LD
SEED = 20250301
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("KRYLOV_RATIOS_OUT")
    if path and RATIOS:
        with open(path, "w") as f:
            for (bar, route), v in sorted(RATIOS.items()):
                f.write("%-34s %-72s %.3f\n" % (bar, route, v))


def record(bar, route, v):
    RATIOS[(bar, route)] = max(RATIOS.get((bar, route), 0.0), float(v))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def nan_like(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def host(t):
    return t.cpu().numpy()


class Recorder:
    """The callbacks of one solve on the torch twin of a krylov_ref.Op; `events` is the solve as the solver's callers saw it."""

    def __init__(self, op, x, reduce=None):
        self.op, self.xptr, self.reduce, self.events = op, x.data_ptr(), reduce, []
        op.reset()

    def A(self, xin, yout):
        yout.copy_(self.op.A_torch(xin))
        self.events.append(("A", xin.numel() > 0 and xin.data_ptr() == self.xptr, xin.clone(), yout.clone()))   # w is updated in place later

    def M(self, vin, zout):
        zout.copy_(self.op.M_torch(vin))
        self.events.append(("M", vin.clone(), zout.clone()))

    def reduce_fn(self):
        def red(ctx, ptr, count, stream):
            try:
                t = sp.device_view(ptr, count)
                self.events.append(("R", int(count), t.clone()))          # the device's own (local) sums
                if self.reduce == "double":
                    t.mul_(2.0)                                          # two ranks holding identical halves
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return 5
        self._cb = sp.REDUCE_FN(red)
        return C.cast(self._cb, C.c_void_p)


def device_solve(c, op, b, x0, rtol=1e-300):
    """One recorded solve of case c.  Returns (x, iterations, reason, residual, events)."""
    cls, n, r, mi, exact, red, prec, xnz, gen = c
    sp.set_option("krylov_exact_norm", exact)
    ks = None
    try:
        ks = sp.Fgmres(n, restart=r, rtol=rtol, max_it=mi)
        bd = dev(b)
        xd = dev(x0) if xnz else nan_like(n)
        rec = Recorder(op, xd, red)
        if red:
            ks.set_reduce_raw(rec.reduce_fn(), None)
        ks.solve(rec.A, bd, xd, M=rec.M if prec else None, x_nonzero=bool(xnz))
        torch.cuda.synchronize()
        return host(xd), ks.iterations, ks.reason, ks.residual, rec.events
    finally:
        sp.set_option("krylov_exact_norm", 0)
        if ks is not None:
            ks.destroy()


def parse(events, c):
    """The recorded calls of a solve that ran to its iteration limit (nothing speculative), as krylov_ref.check_trace reads them.
    The order of the calls is itself checked: residual evaluations read x, the operator reads the preconditioner's output."""
    cls, n, m, mi, exact, red, prec, xnz, gen = c
    pos = [0]

    def take(kind, count=None):
        assert pos[0] < len(events), "the solve made fewer calls than its iterations need"
        e = events[pos[0]]
        assert e[0] == kind and (count is None or e[1] == count), (pos[0], e[0], e[1] if kind == "R" else None, kind, count)
        pos[0] += 1
        return e
    tr = dict(bnsq=None, cycles=[])
    if red:
        tr["bnsq"] = host(take("R", 1)[2])[0]
    its, first = 0, True
    while n > 0 and its < mi:
        cyc = dict(ax=None, rnsq=None, steps=[])
        if not (first and not xnz):
            e = take("A")
            assert e[1], "a cycle's residual evaluation must read x"
            cyc["ax"] = host(e[3])
            if red:
                cyc["rnsq"] = host(take("R", 1)[2])[0]
        first = False
        cols = min(m, mi - its)
        for j in range(cols):
            st = dict(hcol=None, nsq=None)
            if prec:
                em = take("M")
                ea = take("A")
                assert torch.equal(ea[2], em[2]), "the operator must read z_j = M v_j"
                st["v"], st["z"] = host(em[1]), host(em[2])
            else:
                ea = take("A")
                st["v"] = host(ea[2])
            assert not ea[1]
            st["w"] = host(ea[3])
            if red:
                st["hcol"] = host(take("R", j + 1 if exact else j + 2)[2])
                if exact or j + 1 < cols:
                    st["nsq"] = host(take("R", 1)[2])[0]
            cyc["steps"].append(st)
        its += cols
        tr["cycles"].append(cyc)
    assert pos[0] == len(events), "the solve made %d calls more than its iterations need" % (len(events) - pos[0])
    return tr


_REF = {}


def reference(c):
    """(op, b, x0, long-double solve, restatements) of a case, computed once and left unchanged."""
    if c not in _REF:
        op, b, x0 = kr.case_setup(c, SEED)
        ld, rest = kr.reference_solves(op, b, x0, c[2], c[3], c[4], 2 if c[5] == "double" else 1)
        _REF[c] = (op, b, x0, ld, rest)
    return _REF[c]


def run_case(c):
    cls, n, r, mi, exact, red, prec, xnz, gen = c
    op, b, x0, ld, rest = reference(c)
    dup = 2 if red == "double" else 1
    x, its, reason, resid, events = device_solve(c, op, b, x0)
    tr = parse(events, c)
    got = kr.check_trace(tr, b, exact, dup, bool(red))
    if cls != "ill":
        got["solve_max"], got["solve_2"] = kr.solve_ratios(x, ld["x"], [q["x"] for q in rest])
        if not ld["last_est"] and ld["its"] > 0:
            got["residual"] = kr.scalar_ratio(resid, ld["rnorm"], [q["rnorm"] for q in rest])
    route = kr.case_route(c)
    for k, v in got.items():
        if not (v == 0.0 and k in ("dots", "nsq", "norm", "rnorm", "stored")):       # (not observed / not on this route)
            record({"solve_max": "solve, max-norm (of 16 x restatement)", "solve_2": "solve, 2-norm (of 16 x restatement)",
                    "residual": "residual (of 16 x restatement)"}.get(k, "step %s (fraction of cap)" % k), route, v)
    print(kr.case_id(c), {k: round(v, 3) for k, v in got.items()}, its, reason)
    return dict(x=x, its=its, reason=reason, got=got, tr=tr, ld=ld, rest=rest)


@pytest.mark.parametrize("c", kr.CASES + kr.ILL_CASES, ids=kr.case_id)
def test_every_step_and_the_whole_solve(c):
    out = run_case(c)
    assert (out["its"], out["reason"]) == (out["ld"]["its"], out["ld"]["reason"])
    assert all(v <= 1.0 for v in out["got"].values()), out["got"]


IDENT = [c for c in kr.CASES if c[5] == "ident" and c[:5] + (None,) + c[6:] in kr.CASES]


@pytest.mark.parametrize("c", IDENT, ids=kr.case_id)
def test_identity_reduce_reproduces_the_solve_without_one(c):
    """A communicator of one rank: the same V_0 and the same first w bit for bit, the first stored vector within the step bar of the
    truth formed from the OTHER solve's inputs, and both solutions within the whole-solve bar of the same truth."""
    plain = c[:5] + (None,) + c[6:]
    assert len(IDENT) >= 2
    a, p = run_case(c), run_case(plain)
    sa, sp_ = a["tr"]["cycles"][0]["steps"], p["tr"]["cycles"][0]["steps"]
    assert np.array_equal(sa[0]["v"], sp_[0]["v"]) and np.array_equal(sa[0]["w"], sp_[0]["w"])
    T_c = kr.step_counts(c[1], c[4], True)[2]
    t = kr.step_truth(sp_[0]["v"].astype(LD)[None], sp_[0]["w"].astype(LD), c[4])
    q, phi = kr.stored_ratio(sa[1]["v"], t, 1, T_c)
    assert q <= 1.0, q
    assert (a["its"], a["reason"]) == (p["its"], p["reason"])
    for o in (a, p):
        assert o["got"]["solve_max"] <= 1.0 and o["got"]["solve_2"] <= 1.0, o["got"]


@pytest.mark.parametrize("n", [4097, 4098, 262921])
def test_eigenvector_rhs_ends_after_one_iteration(n):
    """b a multiple of the constant vector and a constant: w is parallel to V_0 element by element, e2 clamps, the solve must end at one
    iteration with x = b / lambda.  lambda is read off the operator's own recorded output (its roundings are not the solver's).
    Bar (krylov_ref: eigen): |x_e - b_e / lambda| <= (T_dot + 6) 2^-53 |b_e / lambda|."""
    op = kr.Op(n, SEED, kind="circ")
    b = kr.rhs("const", n, SEED)
    ks = sp.Fgmres(n, restart=5, rtol=1e-10, max_it=20)
    bd, xd = dev(b), nan_like(n)
    rec = Recorder(op, xd)
    ks.solve(rec.A, bd, xd)
    torch.cuda.synchronize()
    its, reason = ks.iterations, ks.reason
    ks.destroy()
    v, w = host(rec.events[0][2]).astype(LD), host(rec.events[0][3]).astype(LD)
    assert np.all(v == v[0]) and np.all(w == w[0])
    lam = w[0] / v[0]
    want = b.astype(LD) / lam
    q = kr.ratio(np.abs(host(xd).astype(LD) - want), LD(kr.eigen_cap(n) * kr.U53) * np.abs(want))
    record("eigenvector x (fraction of cap)", "one-reduction | no reduce | n = %d" % n, q)
    print("eigen", n, q, its, reason)
    assert (its, reason) == (1, 2)
    assert q <= 1.0, q


def _clean(n, exact, ks=None):
    """A clean solve (fixed preconditioner, to convergence) on the given or a fresh handle: (x, iterations, reason, residual)."""
    op = kr.Op(n, SEED + 5, prec="fixed")
    b = kr.rhs("normal", n, SEED + 6)
    own = ks is None
    if own:
        ks = sp.Fgmres(n, restart=9, rtol=1e-11, max_it=60)
    xd = nan_like(n)
    rec = Recorder(op, xd)
    ks.solve(rec.A, dev(b), xd, M=rec.M)
    torch.cuda.synchronize()
    out = (xd.clone(), ks.iterations, ks.reason, ks.residual)
    if own:
        ks.destroy()
    return out


@pytest.mark.parametrize("n,exact", [(4097, 0), (4098, 0), (4098, 1)])
def test_breakdown_zero_rhs_and_nan_leave_the_handle_clean(n, exact):
    sp.set_option("krylov_exact_norm", exact)
    try:
        fresh = _clean(n, exact)
        assert fresh[2] == 2 and 9 < fresh[1] < 60              # more than one cycle
        ks = sp.Fgmres(n, restart=9, rtol=1e-11, max_it=60)
        b = dev(kr.rhs("normal", n, SEED + 7))

        def same_as_fresh():
            again = _clean(n, exact, ks)
            assert torch.equal(again[0], fresh[0]) and again[1:] == fresh[1:], (again[1:], fresh[1:])
        # A = 0: breakdown at the first column, x (never written) cleared
        xd = nan_like(n)
        ks.solve(lambda x, y: y.zero_(), b, xd)
        assert ks.reason == -9 and ks.iterations == 0 and float(xd.abs().max()) == 0.0
        same_as_fresh()
        # b = 0
        xd = nan_like(n)
        rec = Recorder(kr.Op(n, SEED + 5), xd)
        ks.solve(rec.A, torch.zeros_like(b), xd)
        assert ks.iterations == 0 and ks.reason > 0 and float(xd.abs().max()) == 0.0 and not rec.events
        same_as_fresh()
        # the operator's third product is NaN (arithmetic only)
        xd = nan_like(n)
        rec = Recorder(kr.Op(n, SEED + 5), xd)

        def a_nan(x, y):
            rec.A(x, y)
            if len(rec.events) == 3:
                y.fill_(float("nan"))
        ks.solve(a_nan, b, xd)
        assert ks.reason == -9 and ks.iterations == 2
        same_as_fresh()
        ks.destroy()
    finally:
        sp.set_option("krylov_exact_norm", 0)


@pytest.mark.parametrize("entry", ["python", "c_entry"])
def test_the_same_solve_twice_gives_the_same_bits(entry):
    """Twice on one handle and once on a second: the same bits and the same iteration count.  "c_entry": EllipticOp's C entry point, no
    Python between the launches."""
    if entry == "python":
        n = 4098
        kop = kr.Op(n, SEED + 8, prec="vary")
        op = None
    else:
        op = sp.EllipticOp((20, 18, 16))
        n = op.global_size
    b = dev(np.random.default_rng(SEED + 9).standard_normal(n))
    restart = 9 if op is None else 30
    handles = [sp.Fgmres(n, restart=restart, rtol=1e-10 if op is None else 1e-8, max_it=4000) for _ in range(2)]
    runs = []
    for ks in (handles[0], handles[0], handles[1]):
        xd = nan_like(n)
        if op is None:
            rec = Recorder(kop, xd)
            ks.solve(rec.A, b, xd, M=rec.M)
        else:
            ks.solve(op, b, xd)
        torch.cuda.synchronize()
        runs.append((xd, ks.iterations, ks.reason, ks.residual))
    assert runs[0][2] == 2 and runs[0][1] > restart                 # converged, over more than one cycle
    for q in runs[1:]:
        assert torch.equal(q[0], runs[0][0]) and q[1:] == runs[0][1:], (q[1:], runs[0][1:])
    for ks in handles:
        ks.destroy()
    if op is not None:
        op.destroy()


def test_every_route_of_the_table_was_named():
    """Every (step, reduction, load width, trips) the case table is there to reach has a case."""
    routes = {(c[4], c[5], c[1] % 2, kr.trips(c[1], kr.RB * kr.ST, c[1] % 2 == 0) - (c[1] % 2 == 0)) for c in kr.CASES if c[1] > 3}
    for exact in (0, 1):
        for par in (0, 1):
            assert any(r[0] == exact and r[2] == par and r[3] == 2 for r in routes), (exact, par)
            for red in (None, "double", "ident"):
                assert any(r[:3] == (exact, red, par) for r in routes) or red == "ident", (exact, red, par)
