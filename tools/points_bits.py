#!/usr/bin/env python3
"""Output bits of everything that goes through the kernels of ChebPoints (k_points_rows, k_points_frows, k_points_contract,
k_points_grad1, k_points_spread; DESIGN.md sections 10e, 10k, 10m, 10o): rows and drows at every lane-group size of either basis
(uniform points, the nodes, their nextafter neighbours, a NaN and -Inf, a periodic direction's nodes shifted by whole periods), and on
handles that reach every route of the scattered calls -- d = 1 direct and copied, the 64- and the 256-thread contraction, aligned
and unaligned pair loads, d known at compile time or not, BM = 64 and 128 in spread, the chunk of one point, handles with periodic
directions -- eval, eval(deriv) for every unit multi-index and a mixed one, eval_grad with and without value and scale, spread
plain / delta / accumulate / deriv with the option points_spread_pass at 0 and 26, and eval_grid with a shrinking and a growing
direction, plain and with deriv, for npts in {1, chunk, chunk + 1}; first of all what the entry points refuse, word for word, and
the host rows of the three *_matrix_host entries.  One line per case -- a shape, its periodic mask and its
field count -- with one SHA-256 over the output bytes of all its calls, so a pair of runs stays short enough to commit; --all prints
a line per output as well, which is what to look at when two case lines differ.  Inputs from a fixed NumPy seed.  The script
compares nothing: run it on two builds of the library, each in a fresh process, and diff the outputs
    python tools/points_bits.py > new.txt
    CHEBHIP_LIB_PATH=/elsewhere/libchebhip.so python tools/points_bits.py > parent.txt
(profiles/points/bits_parent.txt and bits_new.txt are such a pair).  A refusal is an output; a device error ends the run.
usage: points_bits.py [--all]"""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import __graft_entry__ as ge
sp = ge.load()
SEED = 20261020
ALL = "--all" in sys.argv[1:]
CASE = [None]                                    # the running hash of the case at hand

ROWS_CGL = [2, 17, 64, 65, 257]
ROWS_PERIODIC = [2, 9, 16, 65, 256]
# (dims, fields): d = 1 direct and copied; 64-thread contraction, aligned rows; odd last extent; 256 threads and BM = 128; DC == 0 twice
SCATTERED = [((17,), 3), ((4, 257), 2), ((5, 7, 9), 16), ((66, 65, 64), 3), ((6, 5, 4, 3), 2), ((3, 2, 4, 3, 2), 1)]
MASKS_3 = [(1, 0, 1), (0, 1, 0), (1, 1, 1)]
ONE_POINT = ((2, 1024, 1024, 2), 1)              # tests/test_gpu_points_deriv.py::test_a_chunk_of_one_point: chunk == 1, H == 0
SCALE = (2.0, 0.5, 3.0, 1.25, 0.75)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def emit(tag, what, fn):
    try:
        line = "%s %s %s" % (tag, what, fn())
    except (sp.ChebhipError, ValueError) as e:   # (a refusal is an output too: both builds must give the same one)
        if getattr(e, "code", 0) == 5:           # CHEBHIP_ERR_DEVICE
            raise
        line = "%s %s refused: %s" % (tag, what, e)
    CASE[0].update(line.encode())
    if ALL:
        print(line, flush=True)


def case_line(name):
    print("%s %s" % (name, CASE[0].hexdigest()), flush=True)


def rows_case(n, periodic, rng):
    CASE[0] = hashlib.sha256()
    tag = "rows n=%d %s" % (n, "periodic" if periodic else "cgl")
    h = sp.ChebPoints((n,), 1, periodic=(True,) if periodic else None)
    nodes = sp.fourier_nodes(n) if periodic else sp.cgl_nodes(n)
    xs = [rng.uniform(-1.2, 1.2, 50), nodes, np.nextafter(nodes, 2.0), np.nextafter(nodes, -2.0), [np.nan, -np.inf]]
    if periodic:
        xs += [nodes + 2.0, nodes - 4.0, nodes + 1024.0]
    x = dev(np.concatenate([np.asarray(v, dtype=np.float64) for v in xs]))
    emit(tag, "rows", lambda: sha(h.rows(0, x)))
    emit(tag, "drows", lambda: sha(h.drows(0, x)))
    emit(tag, "rows of one", lambda: sha(h.rows(0, x[:1])))
    h.destroy()
    case_line(tag)


def points_of(dims, mask, npts, rng):
    """Uniform points, a little past the walls (a CGL direction extrapolates, a periodic one wraps); the first is a node."""
    pts = rng.uniform(-1.05, 1.05, (npts, len(dims)))
    pts[0] = [(sp.fourier_nodes(n) if p else sp.cgl_nodes(n))[n // 2] for n, p in zip(dims, mask)]
    return pts


def scattered_case(dims, nf, mask, rng, counts=None):
    CASE[0] = hashlib.sha256()
    d = len(dims)
    name = "%s mask=%s nf=%d" % ("x".join(map(str, dims)), "".join(map(str, mask)), nf)
    made = []
    emit(name, "create", lambda: made.append(sp.ChebPoints(dims, nf, periodic=mask if any(mask) else None)) or "chunk %d" % made[0].chunk)
    if not made:
        return case_line(name)
    h = made[0]
    C = h.chunk
    u = dev(rng.standard_normal(h.size()))
    units = [tuple(int(k == c) for k in range(d)) for c in range(d)]
    mixed = tuple(int(k in (0, d - 1)) for k in range(d))
    derivs = units + ([mixed] if d > 1 else [])
    scale = SCALE[:d]
    for npts in counts or (1, C, C + 1):
        tag = "%s npts=%d" % (name, npts)
        pts = dev(points_of(dims, mask, npts, rng))
        s = dev(rng.standard_normal((nf, npts)))
        emit(tag, "eval", lambda: sha(h.eval(u, pts)))
        for dv in derivs:
            emit(tag, "eval deriv=%s" % "".join(map(str, dv)), lambda: sha(h.eval(u, pts, deriv=dv)))
        for value in (False, True):
            for sc in (None, scale):
                emit(tag, "eval_grad value=%d scale=%d" % (value, sc is not None), lambda: sha(h.eval_grad(u, pts, value=value, scale=sc)))
        for size in (0, 26):
            sp.set_option("points_spread_pass", size)
            try:
                g = torch.empty(h.size(), dtype=torch.float64, device="cuda")
                emit(tag, "spread pass=%d" % size, lambda: sha(h.spread(s, pts, out=g)))
                emit(tag, "spread pass=%d accumulate" % size, lambda: sha(h.spread(s, pts, out=g, accumulate=True)))
                emit(tag, "spread pass=%d delta" % size, lambda: sha(h.spread(s, pts, delta=True)))
                emit(tag, "spread pass=%d deriv" % size, lambda: sha(h.spread(s, pts, deriv=derivs[-1])))
                emit(tag, "spread pass=%d delta deriv accumulate" % size,
                     lambda: sha(h.spread(s, pts, out=g, accumulate=True, delta=True, deriv=units[0])))
            finally:
                sp.set_option("points_spread_pass", 0)
    # tensor grids: direction 0 shrinks, the last one grows (d = 1: one grid each); the large shape keeps its middle directions short
    big = h.size() > (1 << 20)
    grids = [(dims[0] - 1,), (dims[0] + 1,)] if d == 1 else \
        [(max(dims[0] - 1, 1),) + tuple(2 if big else n for n in dims[1:-1]) + (dims[-1] + 1,)]
    for m in grids:
        coords = [dev(np.sort(rng.uniform(-1.0, 1.0, mk))) for mk in m]
        tag = "%s grid=%s" % (name, "x".join(map(str, m)))
        h.reserve_grid(m)
        emit(tag, "eval_grid", lambda: sha(h.eval_grid(u, coords)))
        emit(tag, "eval_grid deriv", lambda: sha(h.eval_grid(u, coords, deriv=derivs[-1])))
    h.destroy()
    case_line(name)


def refusals_case(rng):
    """What the entry points refuse, word for word."""
    CASE[0] = hashlib.sha256()
    tag = "refusals"
    emit(tag, "periodic extent", lambda: sp.ChebPoints((300, 4, 3), 1, periodic=(1, 0, 0)))
    emit(tag, "fields", lambda: sp.ChebPoints((5, 4), 17))
    h = sp.ChebPoints((5, 4, 3), 2, periodic=(0, 1, 0))
    u, pts, s = dev(rng.standard_normal(h.size())), dev(rng.uniform(-1, 1, (7, 3))), dev(rng.standard_normal((2, 7)))
    emit(tag, "rows direction", lambda: sha(h.rows(3, pts[:, 0].contiguous())))
    emit(tag, "drows direction", lambda: sha(h.drows(-1, pts[:, 0].contiguous())))
    for what, fn in (("eval", lambda dv: h.eval(u, pts, deriv=dv)), ("spread", lambda dv: h.spread(s, pts, deriv=dv)),
                     ("eval_grid", lambda dv: h.eval_grid(u, [pts[:, k].contiguous() for k in range(3)], deriv=dv)),
                     ("eval of no points", lambda dv: h.eval(u, pts[:0], deriv=dv))):
        emit(tag, what + " deriv value", lambda: sha(fn((0, 2, 0))))
        emit(tag, what + " deriv length", lambda: sha(fn((0, 1))))
    emit(tag, "eval overlap", lambda: sha(h.eval(u, pts, out=u[:14].reshape(2, 7))))
    emit(tag, "eval_grad scale", lambda: sha(h.eval_grad(u, pts, scale=(1.0, float("inf"), 1.0))))
    emit(tag, "spread accumulate", lambda: sha(h.spread(s, pts, accumulate=True)))
    emit(tag, "spread of no points", lambda: sha(h.spread(s[:, :0], pts[:0])))
    emit(tag, "eval_grid past the reserve", lambda: sha(h.eval_grid(u, [dev(np.linspace(-1, 1, 9)) for _ in range(3)])))
    for name, fn in (("interp_matrix", sp.interp_matrix), ("deriv_matrix", sp.deriv_matrix)):       # the three *_matrix_host entries
        for periodic in (False, True):
            emit(tag, "%s periodic=%d n" % (name, periodic), lambda: fn(1, [0.0], periodic=periodic).tobytes().hex())
            emit(tag, "%s periodic=%d large n" % (name, periodic), lambda: fn(257, [0.0], periodic=periodic).tobytes().hex()[:16])
            emit(tag, "%s periodic=%d no point" % (name, periodic), lambda: fn(5, [], periodic=periodic).tobytes().hex())
            emit(tag, "%s periodic=%d rows" % (name, periodic),
                 lambda: hashlib.sha256(fn(6, [-1.0, 0.3, float("nan"), 1.5], periodic=periodic).tobytes()).hexdigest())
    h.destroy()
    case_line(tag)


def main():
    assert torch.cuda.is_available(), "points_bits needs a GPU"
    refusals_case(np.random.default_rng([SEED, 3]))
    for q, (n, periodic) in enumerate([(n, False) for n in ROWS_CGL] + [(n, True) for n in ROWS_PERIODIC]):
        rows_case(n, periodic, np.random.default_rng([SEED, 0, q]))
    cases = []
    for dims, nf in SCATTERED:
        cases.append((dims, nf, (0,) * len(dims)))
        if len(dims) == 3:
            cases += [(dims, nf, m) for m in MASKS_3 if all(n <= 256 for n, p in zip(dims, m) if p)]
    cases.append(((4, 5, 4, 6), 2, (1, 0, 1, 0)))
    for q, (dims, nf, mask) in enumerate(cases):
        scattered_case(dims, nf, mask, np.random.default_rng([SEED, 1, q]))
    dims, nf = ONE_POINT
    scattered_case(dims, nf, (0,) * len(dims), np.random.default_rng([SEED, 2]), counts=(1, 2))


if __name__ == "__main__":
    main()
