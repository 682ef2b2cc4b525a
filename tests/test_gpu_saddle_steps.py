"""The Stokes block preconditioners (csrc/saddle.hip, StokesPCApply0..3) against long-double truth in the configurations they run in
(saddle_ref.py; the host side is test_saddle_host.py).

  a. every case of saddle_ref.cases(): the default limits (4 velocity, 3 Schur iterations, svel preonly) on nine small shapes -- one
     and two interior nodes, odd and even pressure and velocity counts, last-dimension lines of 68 and 129 points -- for the four
     kinds and three states (eta == 1, variable eta, a Newton state with eta' and strain); a truncated svel GMRES, no Jacobi scaling,
     pc_sweeps = 2 (the node-major route with the inner GMRES on the stencil), the node-major option, preonly velocity solves with
     one Schur iteration, and inner solves that end on their tolerance, on two shapes.  Output vectors arrive as NaN.  Every case
     asserts: the max-norm and 2-norm error of the velocity and of the pressure part against the truth at most 16 x the larger error
     of the two double restatements; the inner iteration counts equal to the truth's; the pressure zero-mean to the derived bar.
  b. (43, 42, 44), 68 880 pressure unknowns (the mean's second grid-stride trip): anchored in double, the device's difference from
     restatement A at most 16 |A - B|.
  c. on one handle: the same apply twice, pc_sweeps 2 -> 0, the type through 0 .. 3 and back: the same bits.

Where SADDLE_RATIOS_OUT names a file the worst ratio per bar and route is written there (profiles/saddle/ratios.txt)."""
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import krylov_ref as kr
import oracle_lib as orc
import saddle_ref as sr

pytestmark = pytest.mark.gpu
sp = ge.load()
LD = np.longdouble
SEED = 20260101                # shared with test_saddle_host.py
NT = 16
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("SADDLE_RATIOS_OUT")
    if path and RATIOS:
        with open(path, "w") as f:
            for (bar, route), v in sorted(RATIOS.items()):
                f.write("%-44s %-40s %.3f\n" % (bar, route, v))


def record(bar, route, v):
    RATIOS[(bar, route)] = max(RATIOS.get((bar, route), 0.0), float(v))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def nan_like(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def make_op(c):
    """The operator of a case with its state set, and the state read back: the doubles the device holds."""
    dims, kind, sname, name = c
    d = len(dims)
    op = sp.StokesOp(dims)
    st = sr.make_state(dims, sname, sr.case_seed(c, SEED))
    if st is not None:
        eta, deta, strain = st
        op.set_state(0, eta)
        if deta is not None:
            op.set_state(1, deta)
            for j in range(d):
                op.set_state(2 + j, strain[j])
        back = [op.get_state(w) for w in range(2 + d)]
        st = (back[0], None if deta is None else back[1], None if deta is None else np.stack(back[2:]))
    return op, st


def make_pc(op, kind, cfg, node_major=False):
    sp.set_option("saddle_node_major", 1 if node_major else 0)
    try:
        pc = sp.StokesSaddlePc(op, kind, vel=cfg["vel"], schur=cfg["schur"], svel=cfg["svel"], pc_sweeps=cfg["pc_sweeps"],
                               schur_jacobi=cfg["schur_jacobi"])
    finally:
        sp.set_option("saddle_node_major", 0)
    pc.setup()
    return pc


def device_apply(pc, x):
    y = pc.apply(dev(x), nan_like(x.size))
    torch.cuda.synchronize()
    return y.cpu().numpy(), pc.inner_iterations


def route(c):
    dims, kind, sname, name = c
    return "%s | %s" % (name, "x".join(map(str, dims)))


def check_mean(c, y):
    yp = sr.split(y, len(c[0]))[1]
    m, bar = sr.mean_of(yp), sr.mean_bar(yp)
    q = kr.ratio(m, bar)
    record("zero mean (fraction of bar)", route(c), q)
    return q


@pytest.mark.parametrize("c", sr.cases(), ids=sr.case_id)
def test_block_preconditioner_against_truth(c):
    dims, kind, sname, name = c
    d = len(dims)
    op, st = make_op(c)
    pc = None
    try:
        r = sr.reference(sp, c, SEED, state=st)
        pc = make_pc(op, kind, r["cfg"], node_major=(name == "C5"))
        y, its = device_apply(pc, r["x"])
    finally:
        if pc is not None:
            pc.destroy()
        op.destroy()
    got = sr.part_ratios(y, r["ld"]["y"], [q["y"] for q in r["rest"]], d)
    qm = check_mean(c, y)
    for k, v in got.items():
        record({"v_max": "velocity, max-norm (of 16 x restatement)", "v_2": "velocity, 2-norm (of 16 x restatement)",
                "p_max": "pressure, max-norm (of 16 x restatement)", "p_2": "pressure, 2-norm (of 16 x restatement)"}[k], route(c), v)
    print(sr.case_id(c), {k: round(v, 3) for k, v in got.items()}, "mean %.3f" % qm, "its", its, r["ld"]["its"], "gap %.3g" % sr.gap(r["ld"]["hist"]))
    assert np.all(np.isfinite(y))
    assert its == r["ld"]["its"], (its, r["ld"]["its"])
    assert all(v <= 1.0 for v in got.values()), got
    assert qm <= 1.0, qm
    if dims == (3, 3):
        assert not np.any(sr.split(y, d)[1])                     # one pressure unknown: the zero-mean subspace is {0}


_LARGE = {}


def large_reference(c, st):
    if c not in _LARGE:
        dims, kind, sname, name = c
        x = sr.case_rhs(c, SEED)
        cfg = sr.case_config(c)
        _LARGE[c] = (x, cfg, sr.apply(sr.oracle_ops(sp, dims, st, orc.DIRECT, "plain", NT), x, kind, cfg, np.float64, kr.dot_pairwise),
                     sr.apply(sr.oracle_ops(sp, dims, st, orc.FAST, "evenodd", NT), x, kind, cfg, np.float64, kr.dot_strided))
    return _LARGE[c]


@pytest.mark.parametrize("c", sr.LARGE_CASES, ids=sr.case_id)
def test_large_shape_against_the_restatements(c):
    """68 880 pressure unknowns: k_mean_partial's second grid-stride trip.  Dense long-double blocks are out of reach: the device's
    difference from restatement A at most 16 |A - B| per part, the counts against A's, the zero-mean bar."""
    dims, kind, sname, name = c
    d = len(dims)
    assert int(np.prod(sr.idims(dims))) > sr.MEAN_RB * sr.MEAN_RT
    op, st = make_op(c)
    pc = None
    try:
        x, cfg, a, b = large_reference(c, st)
        pc = make_pc(op, kind, cfg)
        y, its = device_apply(pc, x)
    finally:
        if pc is not None:
            pc.destroy()
        op.destroy()
    got = sr.pair_ratios(y, a["y"], b["y"], d)
    qm = check_mean(c, y)
    for k, v in got.items():
        record({"v_max": "velocity, max-norm (of 16 |A - B|)", "v_2": "velocity, 2-norm (of 16 |A - B|)",
                "p_max": "pressure, max-norm (of 16 |A - B|)", "p_2": "pressure, 2-norm (of 16 |A - B|)"}[k], route(c), v)
    print(sr.case_id(c), {k: round(v, 3) for k, v in got.items()}, "mean %.3f" % qm, "its", its, a["its"])
    assert its == a["its"] == b["its"]
    assert all(v <= 1.0 for v in got.values()), got
    assert qm <= 1.0, qm


# ----------------------------------------------------------------------------------------------
# on one handle
# ----------------------------------------------------------------------------------------------
HANDLE_CASE = ((10, 9, 8), 0, "jacobian", "C1")


def test_the_same_apply_twice_gives_the_same_bits():
    op, st = make_op(HANDLE_CASE)
    x = sr.rhs(HANDLE_CASE[0], SEED + 7)
    pc = make_pc(op, 0, sr.config())
    try:
        runs = [device_apply(pc, x) for _ in range(2)]
    finally:
        pc.destroy(); op.destroy()
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert np.all(np.isfinite(runs[0][0]))


def test_pc_sweeps_set_back_to_zero_is_a_fresh_handle():
    """Created with pc_sweeps = 2 (node-major route, inner GMRES allocated and used), then stokes_saddle_set_pc_sweeps(0): the bits
    of a handle that never left the component-major route."""
    op, st = make_op(HANDLE_CASE)
    x = sr.rhs(HANDLE_CASE[0], SEED + 7)
    pc, fresh = make_pc(op, 0, sr.config(pc_sweeps=2)), make_pc(op, 0, sr.config())
    try:
        swept = device_apply(pc, x)
        sp._chk(sp.lib().stokes_saddle_set_pc_sweeps(pc._h, 0))
        back = device_apply(pc, x)
        want = device_apply(fresh, x)
    finally:
        pc.destroy(); fresh.destroy(); op.destroy()
    assert np.array_equal(back[0], want[0]) and back[1] == want[1]
    assert not np.array_equal(swept[0], want[0])


def test_type_through_all_kinds_and_back():
    op, st = make_op(HANDLE_CASE)
    x = sr.rhs(HANDLE_CASE[0], SEED + 7)
    pc = make_pc(op, 0, sr.config())
    try:
        first = device_apply(pc, x)
        seen = []
        for kind in (1, 2, 3, 0):
            sp._chk(sp.lib().stokes_saddle_set_type(pc._h, kind))
            seen.append(device_apply(pc, x))
    finally:
        pc.destroy(); op.destroy()
    assert np.array_equal(seen[-1][0], first[0]) and seen[-1][1] == first[1]
    assert all(not np.array_equal(s[0], first[0]) for s in seen[:-1])
