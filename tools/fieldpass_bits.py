#!/usr/bin/env python3
"""Output bits of the one-pass reductions that share csrc/rowpass.h (the pair load, the lanes per row, the folds' tiling) and the
host helpers of csrc/ops.h ("Shared pieces of the field passes"): ChebModal.integrate (with and without v) and
spectrum; ChebReduce.apply on every mask of a shape (rows and cols, sliced and unsliced, with and without v); ChebStats.summary,
histogram (uniform and edges, with and without cond) and cfl; ChebPoints.eval.  Shapes: those of tests/test_gpu_fold.py (1, 64
and 72 workgroups, 33, 64 and 128 slices), an odd last extent (rows on 8-byte boundaries: unaligned pair loads), d = 4, and rows
of more than 128 points.  Inputs: N(0, 1) doubles from a fixed NumPy seed with a -0.0 here and there; the last two fields of a
case with three or more carry a NaN and an Inf.  One line per case with one SHA-256 over the output bytes of all its calls;
--all prints a line per call as well.  The script compares nothing: run it on two builds of the library, each in a fresh
process, and diff the outputs
    python tools/fieldpass_bits.py > new.txt
    CHEBHIP_LIB_PATH=/elsewhere/libchebhip.so python tools/fieldpass_bits.py > parent.txt
(profiles/fieldpass/bits_parent.txt and bits_new.txt are such a pair).  tools/points_bits.py covers ChebPoints in full.
usage: fieldpass_bits.py [--all]"""
import hashlib, itertools, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import __graft_entry__ as ge
sp = ge.load()
SEED = 20261021
ALL = "--all" in sys.argv[1:]

# (dims, fields)
MODAL = [((9, 7, 3), 3), ((91, 90, 3), 3), ((97, 95, 3), 3), ((5, 7, 9), 16), ((6, 5, 4, 3), 2), ((40, 48, 130), 1), ((4, 257), 3)]
REDUCE = [((264, 5), 3), ((512, 5), 3), ((1024, 5), 3), ((5, 7, 9), 3), ((6, 5, 4, 3), 2), ((40, 48, 130), 1), ((4, 257), 3)]
STATS = [((9, 7, 3), 3), ((97, 95, 3), 3), ((5, 7, 9), 4), ((6, 5, 4, 3), 2), ((40, 48, 130), 1), ((66, 65, 64), 3)]
POINTS = [((5, 7, 9), 3), ((6, 5, 4, 3), 2), ((66, 65, 64), 3)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).ravel()).cuda()


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def fields(rng, dims, nf, special=True):
    """nf fields of N(0, 1) with every 37th value -0.0; with three fields or more the last but one has a NaN, the last an Inf."""
    T = int(np.prod(dims))
    u = rng.standard_normal((nf, T))
    u[:, ::37] = -0.0
    if special and nf >= 3:
        u[nf - 2, T // 3] = np.nan
        u[nf - 1, T // 2] = np.inf
    return u


class Case:
    def __init__(self, name):
        self.name, self.h = name, hashlib.sha256()

    def emit(self, what, fn):
        line = "%s %s %s" % (self.name, what, fn())
        self.h.update(line.encode())
        if ALL:
            print(line, flush=True)

    def done(self):
        print("%s %s" % (self.name, self.h.hexdigest()), flush=True)


def name_of(kind, dims, nf):
    return "%s %s nf=%d" % (kind, "x".join(map(str, dims)), nf)


def modal_case(dims, nf, rng):
    c = Case(name_of("modal", dims, nf))
    h = sp.ChebModal(dims, nf)
    u, v = dev(fields(rng, dims, nf)), dev(fields(rng, dims, nf, special=False))
    c.emit("integrate u", lambda: sha(h.integrate(u)))
    c.emit("integrate uv", lambda: sha(h.integrate(u, v)))
    c.emit("integrate uu", lambda: sha(h.integrate(u, u)))
    c.emit("spectrum", lambda: sha(h.spectrum(u)))
    c.emit("spectrum of -0.0", lambda: sha(h.spectrum(torch.full_like(u, -0.0))))
    h.destroy()
    c.done()


def reduce_case(dims, nf, rng):
    c = Case(name_of("reduce", dims, nf))
    d = len(dims)
    u, v = dev(fields(rng, dims, nf)), dev(fields(rng, dims, nf, special=False))
    w = rng.standard_normal(dims[0])
    for mask in itertools.product((0, 1), repeat=d):
        if not any(mask):
            continue
        over = tuple(k for k in range(d) if mask[k])
        h = sp.ChebReduce(dims, nf, over=over)
        tag = "mask=%s slices=%d" % ("".join(map(str, mask)), h.slices)
        c.emit(tag + " u", lambda: sha(h.apply(u)))
        c.emit(tag + " uv", lambda: sha(h.apply(u, v)))
        if mask[0]:
            h.set_weights(0, w)
            c.emit(tag + " u weights", lambda: sha(h.apply(u)))
            h.set_weights(0, None)
            c.emit(tag + " u default again", lambda: sha(h.apply(u)))
        h.destroy()
    c.done()


def stats_case(dims, nf, rng):
    c = Case(name_of("stats", dims, nf))
    d = len(dims)
    h = sp.ChebStats(dims, nf, max_bins=64)
    u, cond = dev(fields(rng, dims, nf)), dev(fields(rng, dims, nf, special=False))
    vel = dev(fields(rng, dims, d, special=False))
    center = dev(rng.standard_normal(nf))
    edges = np.sort(rng.standard_normal(17))
    c.emit("summary", lambda: sha(h.summary(u)))
    c.emit("summary center", lambda: sha(h.summary(u, center)))
    for bins in (7, 64):
        c.emit("histogram uniform bins=%d" % bins, lambda: sha(h.histogram(u, bins, range=(-1.5, 2.0))))
        c.emit("histogram uniform cond bins=%d" % bins, lambda: sha(h.histogram(u, bins, range=(-1.5, 2.0), cond=cond)))
    c.emit("histogram auto range", lambda: sha(h.histogram(u, 16)))
    c.emit("histogram edges", lambda: sha(h.histogram(u, 16, edges=edges)))
    c.emit("histogram edges cond", lambda: sha(h.histogram(u, 16, edges=edges, cond=cond)))
    c.emit("histogram of -0.0 cond", lambda: sha(h.histogram(u, 7, range=(-1.5, 2.0), cond=torch.full_like(u, -0.0))))
    c.emit("cfl", lambda: sha(h.cfl(vel)))
    c.emit("cfl scale", lambda: sha(h.cfl(vel, scale=[2.0 / (k + 1) for k in range(d)])))
    h.set_weights(d - 1, rng.standard_normal(dims[-1]))
    c.emit("summary weights", lambda: sha(h.summary(u)))
    h.set_weights(d - 1, None)
    c.emit("summary default again", lambda: sha(h.summary(u)))
    h.destroy()
    c.done()


def points_case(dims, nf, rng):
    c = Case(name_of("points", dims, nf))
    h = sp.ChebPoints(dims, nf)
    u = dev(fields(rng, dims, nf))
    for npts in (1, 77):
        pts = dev(rng.uniform(-1.0, 1.0, (npts, len(dims)))).view(npts, len(dims))
        c.emit("eval npts=%d" % npts, lambda: sha(h.eval(u, pts)))
        c.emit("eval_grad npts=%d" % npts, lambda: sha(h.eval_grad(u, pts, value=True)))
    h.destroy()
    c.done()


def main():
    assert torch.cuda.is_available(), "fieldpass_bits needs a GPU"
    for q, (run, cases) in enumerate(((modal_case, MODAL), (reduce_case, REDUCE), (stats_case, STATS), (points_case, POINTS))):
        for i, (dims, nf) in enumerate(cases):
            run(dims, nf, np.random.default_rng([SEED, q, i]))


if __name__ == "__main__":
    main()
