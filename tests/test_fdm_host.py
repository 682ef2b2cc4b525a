"""Host side of the per-step checks of the fast-diagonalisation solve (fdm_ref.py; the device side is test_gpu_fdm.py): the
finite-difference line as its host accessor gives it, the two double restatements of the solve against the step bars, and planted
faults in the restatement -- what the bars must catch, and a benign variant they must let through.  No GPU."""
import numpy as np
import pytest

import __graft_entry__ as ge
import oracle_lib as orc
import linewise as lw
import fdm_ref as fr
from conftest import relerr

sp = ge.load()
LD = np.longdouble
SEED = 20241019
OLD_TOL = 1e-9                 # the bar of today's round-trip and spsolve checks (test_gpu_precond.py)
MARGIN = 16.0                  # composite: device error <= MARGIN x the larger restatement error (test_gpu_fdm.py)


@pytest.fixture(scope="module", autouse=True)
def _built():
    ge.build()


@pytest.mark.parametrize("P", [3, 4, 5, 8, 9, 33, 64, 66, 130, 255, 256, 258])
def test_fdpc_line(P):
    """S diag(lam) S^-1 is the 1-D matrix of the oracle, S S^-1 = I, and the modes are laid out by parity.  Bars, first order:
    each of S, lam, S^-1 is rounded once from long double (3 roundings of the majorant |S| |lam| |S^-1|, one more for the long-double
    decomposition itself); the oracle forms an entry of T in double with fewer than 8 roundings.  The mirror images within S and
    S^-1 agree to one unit in the last place (each entry is rounded once from its own long-double value)."""
    S, Si, lam = sp.fdpc_line(P)
    M = P - 2
    m, H = M - 1, (M + 1) // 2
    T = np.asarray(orc.fd_matrix((P,)).todense())
    rec = (S.astype(LD) * lam.astype(LD)[None, :]) @ Si.astype(LD)
    maj = (np.abs(S) * np.abs(lam)[None, :]) @ np.abs(Si)
    # ... and each entry of row i divides by three differences of the nodes around node i, which the oracle (like the reference)
    # holds as cos() in double: a difference of two values <= 1 carries an absolute error of 2 x 2^-53 at most, relative
    # 2 x 2^-53 / gap_i with gap_i the smaller distance from node i to its neighbours (large in the middle of the line, pi^2 / 2n^2
    # at its ends)
    xn = np.cos(np.arange(P) * np.pi / (P - 1))
    gap = np.minimum(xn[:-2] - xn[1:-1], xn[1:-1] - xn[2:])[:, None]
    # ... and the decomposition itself is a long-double eigen-solve: a backward error of M 2^-64 max|T|, normwise as such solvers give it
    assert np.all(np.abs(rec - T).astype(np.float64) <= lw.U53 * (3 * maj + (8 + 3 * 2 / gap) * np.abs(T)) + M * 2.0 ** -64 * np.abs(T).max())
    one = S.astype(LD) @ Si.astype(LD)
    assert np.all(np.abs(one - np.eye(M)).astype(np.float64) <= lw.U53 * 3 * (np.abs(S) @ np.abs(Si)))
    # parity: even modes at p < H (columns of S and rows of S^-1 symmetric), the q-th odd mode at m - q (antisymmetric), exactly
    ulp = lambda a, b: np.all(np.abs(a - b) <= 2.0 ** -52 * np.abs(a))
    assert ulp(S[:, :H], S[::-1, :H]) and ulp(Si[:H], Si[:H, ::-1])
    nq = M - H
    odd = m - np.arange(nq)
    assert ulp(S[:, odd], -S[::-1, odd]) and ulp(Si[odd], -Si[odd, ::-1])
    assert np.all(np.diff(lam[:H]) > 0) and np.all(np.diff(lam[odd]) > 0) and np.all(lam > 0)
    with pytest.raises(sp.ChebhipError):
        sp.fdpc_line(2)
    with pytest.raises(sp.ChebhipError):
        sp.fdpc_line(259)


def _eta(shape, seed):
    return np.exp(np.random.default_rng(seed).uniform(np.log(0.5), np.log(10.0), shape))


def _worst_steps(stages, L, sigma, eta):
    """{mode: worst ratio / cap} over the steps of one restatement run; asserts nothing."""
    d = len(L)
    out = {}
    for mode, k, x, y in fr.stage_checks(stages, L, sigma, eta):
        t, B = fr.step_truth_bound(mode, k, x, L, sigma, eta)
        r, _ = lw.worst(y, t, B)
        cap = fr.step_cap(mode, L[k][0].shape[0], d)
        out[(mode, k)] = max(out.get((mode, k), 0.0), r / cap)
    return out


CASES = [("fd", (12, 10)), ("fd", (34, 20, 18)), ("spectral", (130, 70)), ("spectral", (70, 36, 24)), ("fd", (9,)), ("spectral", (6,) * 5)]


@pytest.mark.parametrize("how", ["plain", "evenodd"])
@pytest.mark.parametrize("kind,dims", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_restatements_meet_the_step_bars(kind, dims, how, capsys):
    """Both double restatements of the solve pass every derived step bar, on noise and on noise scaled per node by 10^+-30, with a
    log-uniform eta and sigma = 1.5 on the spectral line; the ratios (fraction of the cap) are printed."""
    L = fr.lines(sp, kind, dims)
    shape = (2,) + tuple(p - 2 for p in dims)
    eta = _eta(shape[1:], SEED)
    sigma = 1.5 if kind == "spectral" else 0.0
    for name, r in (("noise", np.random.default_rng(SEED + 1).standard_normal(shape)), ("scaled", fr.node_scaled(shape, SEED + 2))):
        z, stages = fr.chain(r, L, sigma, eta, how)
        worst = _worst_steps(stages, L, sigma, eta)
        with capsys.disabled():
            print("\n  %s %s %s %s: " % (kind, "x".join(map(str, dims)), how, name) + ", ".join("%s[%d] %.2f" % (m, k, v) for (m, k), v in sorted(worst.items())), end="")
        for key, v in worst.items():
            assert v <= 1.0, (name, key, v)
        for emax, e2 in fr.errors(z, fr.truth(r, L, sigma, eta)):
            assert e2 < 1e-14                        # (the restatements themselves, normwise: 2e-16 .. 6e-16 on record)


def _bars(z, stages, r, L, sigma, eta, clean):
    """(worst step ratio / cap, composite ratio against MARGIN x the clean restatements' errors) of a faulty run."""
    step = max(_worst_steps(stages, L, sigma, eta).values())
    t = fr.truth(r, L, sigma, eta)
    ez = fr.errors(z, t)
    comp = 0.0
    for f in range(len(ez)):
        for q in range(2):
            comp = max(comp, ez[f][q] / (MARGIN * max(c[f][q] for c in clean)))
    return step, comp, relerr(np.asarray(z), t.astype(np.float64))


def _setup(kind, dims, nf=1, bc=None, sigma=0.0, eta=True, seed=SEED + 7):
    L = fr.lines(sp, kind, dims, bc=bc)
    shape = (nf,) + tuple(p - 2 for p in dims)
    r = np.random.default_rng(seed).standard_normal(shape)
    e = _eta(shape[1:], seed + 1) if eta else None
    t = fr.truth(r, L, sigma, e)
    clean = [fr.errors(fr.chain(r, L, sigma, e, how)[0], t) for how in ("plain", "evenodd")]
    return L, r, e, clean


def test_planted_weight_off_by_1e_11(capsys):
    """One mode's weight wrong by 1e-11 relative: invisible at 1e-9, far outside the scaling step's bar."""
    dims = (34, 20, 18)
    L, r, eta, clean = _setup("fd", dims)
    w = fr.weights(L, 0.0).copy()
    w[0, 0, 0, 0] *= 1.0 + 1e-11                                   # the smoothest mode: the largest weight
    z, stages = fr.chain(r, L, 0.0, eta, "evenodd", w=w)
    step, comp, old = _bars(z, stages, r, L, 0.0, eta, clean)
    with capsys.disabled():
        print("\n  weight 1e-11: step %.3g x cap, composite %.3g x bar, relerr %.3g" % (step, comp, old), end="")
    assert old < OLD_TOL
    assert step > 1.0 and comp > 1.0


def test_planted_dropped_mode_with_a_weight(capsys):
    """All-Neumann, sigma = 0: the mode whose eigenvalue sum is exactly 0 must get weight 0.  A finite weight, here 1e-12 of the
    largest one, passes relerr < 1e-9 and fails the scaling bar (B = 0 there demands an exact 0) and the composite."""
    dims = (20, 70)
    bc = ["neumann", "neumann"]
    L, r, eta, clean = _setup("spectral", dims, bc=bc, eta=False)
    w = fr.weights(L, 0.0).copy()
    assert np.count_nonzero(w == 0) == 1
    z0, st0 = fr.chain(r, L, 0.0, None, "evenodd")
    assert max(_worst_steps(st0, L, 0.0, None).values()) <= 1.0      # the clean run, dropped mode included
    w[w == 0] = 1e-12 * np.sort(w.ravel())[-1]
    z, stages = fr.chain(r, L, 0.0, None, "evenodd", w=w)
    step, comp, old = _bars(z, stages, r, L, 0.0, None, clean)
    with capsys.disabled():
        print("\n  dropped mode: step %.3g x cap, composite %.3g x bar, relerr %.3g" % (step, comp, old), end="")
    assert old < OLD_TOL
    assert step == np.inf and comp > 1.0


def test_planted_eta_from_the_neighbouring_node(capsys):
    """eta shifted by one node on a single plane: no present test sees it (both device routes share the gather); the load-side bar
    and the composite do."""
    dims = (34, 20, 18)
    L, r, eta, clean = _setup("fd", dims)
    bad = eta.copy()
    bad[5] = np.roll(eta[5], 1, axis=1)
    z, stages = fr.chain(r, L, 0.0, None, "evenodd", einv=1.0 / bad)
    step, comp, old = _bars(z, stages, r, L, 0.0, eta, clean)
    with capsys.disabled():
        print("\n  eta shifted: step %.3g x cap, composite %.3g x bar, relerr %.3g" % (step, comp, old), end="")
    assert step > 1.0 and comp > 1.0


def test_planted_weight_of_the_transposed_line(capsys):
    """The weight of line (i, j) taken from (j, i) in one tile of 32 lines of the last direction."""
    dims = (34, 20, 18)
    L, r, eta, clean = _setup("fd", dims)
    w = np.broadcast_to(fr.weights(L, 0.0), (1,) + tuple(p - 2 for p in dims)).copy()
    n0, n1 = w.shape[1], w.shape[2]
    lam0, lam1, lam2 = (l[2] for l in L)
    for line in range(64, 96):
        i, j = divmod(line, n1)
        ii, jj = j % n0, i % n1
        w[0, i, j] = 1.0 / ((lam0[ii] + lam1[jj]) + lam2)
    z, stages = fr.chain(r, L, 0.0, eta, "evenodd", w=w)
    step, comp, old = _bars(z, stages, r, L, 0.0, eta, clean)
    with capsys.disabled():
        print("\n  transposed weights: step %.3g x cap, composite %.3g x bar, relerr %.3g" % (step, comp, old), end="")
    assert step > 1.0 and comp > 1.0


def test_planted_line_left_at_its_input(capsys):
    """One line of a partial last tile keeps its input through the last backward transform."""
    dims = (34, 20, 18)
    L, r, eta, clean = _setup("fd", dims)
    keep = {}

    def hook(name, k, a):
        if name == "scale":
            keep["x"] = a.copy()
        if name == "backward" and k == 2:
            a = a.copy()
            a[0, -1, -1, :] = keep["x"][0, -1, -1, :]
        return a
    z, stages = fr.chain(r, L, 0.0, eta, "evenodd", hook=hook)
    step, comp, old = _bars(z, stages, r, L, 0.0, eta, clean)
    with capsys.disabled():
        print("\n  line left: step %.3g x cap, composite %.3g x bar, relerr %.3g" % (step, comp, old), end="")
    assert step > 1.0 and comp > 1.0


def test_benign_reciprocal_of_reciprocal_passes(capsys):
    """fl(1 / fl(1 / fl(1 / eta))) in place of fl(1 / eta): a different last bit here and there, still inside the counted
    roundings -- every bar lets it through."""
    dims = (34, 20, 18)
    L, r, eta, clean = _setup("fd", dims)
    einv = 1.0 / (1.0 / (1.0 / eta))
    if not np.any(einv != 1.0 / eta):              # (where the three divisions land on fl(1 / eta) everywhere: its neighbour, every 7th node)
        einv.reshape(-1)[::7] = np.nextafter(einv.reshape(-1)[::7], np.inf)
    assert np.any(einv != 1.0 / eta)
    z, stages = fr.chain(r, L, 0.0, None, "evenodd", einv=einv)
    step, comp, old = _bars(z, stages, r, L, 0.0, eta, clean)
    with capsys.disabled():
        print("\n  1/(1/(1/eta)): step %.3g x cap, composite %.3g x bar, relerr %.3g" % (step, comp, old), end="")
    assert step <= 1.0 and comp <= 1.0 and old < OLD_TOL
