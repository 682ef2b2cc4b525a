"""cheb_stats_* on the device (ChebStats): summary, histogram and cfl against the long-double twin of stats_ref.py.  Moments and
masses within the derived bars, every slot of every field; slots, counts, extrema, indices and NaN counts exactly; cfl bit for
bit against its double restatement and within (d + 2) U of the long-double sum; isolation of NaN and Inf between fields and
between slots; cross-checks against ChebModal.integrate; run-to-run and stream-to-stream bits; the interface and the two
solve.py wrappers."""
import functools
from importlib import import_module

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import stats_ref as ref

pytestmark = pytest.mark.gpu
sp = ge.load()
solve = import_module(sp.__name__ + ".solve")
SEED = 20241102
LD = np.longdouble
U = 2.0 ** -53

# the smallest shapes that reach every path: rows of 2 .. 1024 points, an odd field size (field 1 starts 8-byte aligned), one to
# five directions, several workgroups and the folds ((96, 97, 95): 108 workgroups in summary / cfl and in histogram)
CASES = [((2,), 16), ((5,), 3), ((7, 3), 3), ((3, 2, 2, 3, 5), 1), ((129, 130), 3), ((33, 34, 35), 16), ((1024,), 16),
         ((96, 97, 95), 1)]
NBINS = [1, 2, 63, 64, 65, 256, 1024]
ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).ravel()).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def data(dims, nf):
    """The inputs of a case, made once and left unchanged: N(0, 1) fields u and c, u sorted per field."""
    rng = np.random.default_rng(SEED + sum(dims) + nf)
    T = int(np.prod(dims))
    u, c = rng.standard_normal((nf, T)), rng.standard_normal((nf, T))
    return dict(u=u, c=c, sorted=np.sort(u, axis=1), T=T, ws=ref.default_weights(dims))


@functools.lru_cache(maxsize=None)
def handle(dims, nf):
    return sp.ChebStats(dims, nf, max_bins=1024)


def test_geometry():
    """(96, 97, 95) runs several workgroups per field in both kernels, so the folds add more than one partial result."""
    h = handle((96, 97, 95), 1)
    assert h.size(0) == 96 * 97 * 95 and h.size(1) == 9 and h.size(2) == 1024 and h.size(3) > 4 and h.size(4) > 4
    assert handle((2,), 16).size(3) == 1 and handle((2,), 16).size(4) == 1


# ---- 1. summary -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,nf", CASES, ids=ids)
def test_summary_bar(dims, nf):
    """N(0, 1) about 0; about the mean of a previous summary, taken on the device without a sync; about a large centre (the
    powers cancel nothing: the bar is in terms of |u - c|^p); with all-ones weights, where M_1 = sum (u - c)."""
    d = data(dims, nf)
    h = handle(dims, nf)
    u = dev(d["u"])
    s0 = h.summary(u)
    c_dev = (s0[:, 5] / 2.0 ** len(dims)).contiguous()               # the volume of [-1, 1]^d is 2^d
    s1 = h.summary(u, center=c_dev)
    c_big = np.linspace(-3.0, 5.0, nf)
    s2 = h.summary(u, center=dev(c_big))
    worst = 0.0
    for what, out, c in (("c = 0", s0, None), ("c = mean", s1, host(c_dev)), ("c = -3..5", s2, c_big)):
        r = ref.summary_ratio(dims, nf, host(out), ref.summary_truth(dims, nf, d["ws"], d["u"], c))
        print("stats-ratio summary %s nf %d %s: %.3g of the bar" % (ids(dims), nf, what, r))
        assert r <= 1.0, (what, r)
        worst = max(worst, r)
    ones = [np.ones(n) for n in dims]
    for k in range(len(dims)):
        h.set_weights(k, ones[k])
    try:
        so = host(h.summary(u, center=c_dev))
    finally:
        for k in range(len(dims)):
            h.set_weights(k, None)
    r = ref.summary_ratio(dims, nf, so, ref.summary_truth(dims, nf, ones, d["u"], host(c_dev)))
    assert r <= 1.0
    plain = (d["u"].astype(LD) - host(c_dev).astype(LD)[:, None]).sum(axis=1)
    bar = (d["T"] + 6) * U * np.abs(d["u"] - host(c_dev)[:, None]).sum(axis=1)
    assert (np.abs(so[:, 5].astype(LD) - plain).astype(np.float64) <= bar).all()
    print("stats-ratio summary %s nf %d: worst %.3g" % (ids(dims), nf, max(worst, r)))
    assert (bits(host(h.summary(u))) == bits(host(s0))).all()         # the default weights are back
    assert (bits(host(u)) == bits(d["u"].ravel())).all()


@pytest.mark.parametrize("dims,nf", [((5,), 3), ((7, 3), 3), ((129, 130), 3), ((96, 97, 95), 1)], ids=ids)
def test_summary_extrema(dims, nf):
    """Ties take the first index (in one row, across rows, across workgroups); -0.0 and +0.0 compare equal and the element found
    keeps its bits; +-Inf count as values; denormals; NaN at the first, a middle and the last element; all-NaN fields."""
    d = data(dims, nf)
    T = d["T"]
    h = handle(dims, nf)
    spots = sorted({0, 1, T // 3, T // 2 + 1, T - 2, T - 1})
    variants = []
    for a, b in ((spots[1], spots[-2]), (spots[0], spots[-1]), (spots[2], spots[3])):
        u = d["u"].copy()
        u[:, [a, b]] = 9.0                                            # max tie: a is first
        u[0, [a, b]] = -9.0                                           # field 0: a min tie instead
        variants.append(u)
    z = np.zeros((nf, T))
    z[:, T // 2] = -0.0                                               # all equal: index 0, whose bits are +0.0
    variants.append(z)
    z = np.zeros((nf, T))
    z[:, 0] = -0.0
    variants.append(z)                                                # ... and here -0.0
    u = d["u"].copy()
    u[:, spots[2]] = np.inf
    u[0, spots[3]] = -np.inf
    u[-1, spots[1]] = 5e-324
    variants.append(u)
    dn = np.full((nf, T), 5e-324)                                     # subnormal: the extrema are exact, the products underflow
    dn[:, T - 1] = -5e-324
    dn[:, T // 2] = 1e-320
    variants.append(dn)
    subnormal = len(variants) - 1
    for i in (0, T // 2, T - 1):
        u = d["u"].copy()
        u[0, i] = np.nan
        variants.append(u)
    u = d["u"].copy()
    u[nf - 1, :] = np.nan                                             # all NaN: +Inf, -Inf, -1, -1
    variants.append(u)
    for n, u in enumerate(variants):
        out = host(h.summary(dev(u)))
        tr = ref.summary_truth(dims, nf, d["ws"], u)
        # the issue's bar as it stands for every variant but one: the field of subnormal values alone gets the format's underflow
        # term on top (stats_ref.summary_ratio says why); no other input of this file is compared with it
        assert ref.summary_ratio(dims, nf, out, tr, underflow=n == subnormal) <= 1.0, n
    assert out[nf - 1, 0] == np.inf and out[nf - 1, 1] == -np.inf and out[nf - 1, 2] == -1 and out[nf - 1, 3] == -1
    assert out[nf - 1, 4] == T and np.isnan(out[nf - 1, 5:]).all()


# ---- 2. histogram ---------------------------------------------------------------------------------------------------------------
def run_hist(h, dims, nf, d, u, nbins, spec, edges=False, cond=None):
    """One call against the twin: the worst error / bar (inf if anything exact is off)."""
    sd = dev(spec)
    out = h.histogram(dev(u), nbins, edges=sd if edges else None, range=None if edges else sd,
                      cond=None if cond is None else dev(cond))
    slots = ref.field_slots(nf, u, nbins, spec, edges)
    return ref.histogram_ratio(dims, nf, nbins, host(out), ref.histogram_truth(dims, nf, d["ws"], slots, nbins, cond)), host(out)


@pytest.mark.parametrize("nbins", NBINS)
@pytest.mark.parametrize("dims,nf", CASES, ids=ids)
def test_histogram_bar(dims, nf, nbins):
    """N(0, 1) over (-2.5, 3) (underflow and overflow are populated); the same sorted (a whole wave in one bin); dealt round-robin
    over the bins (every lane in another bin); with a second field; by edges (unequal bins, one of them empty)."""
    d = data(dims, nf)
    h = handle(dims, nf)
    T = d["T"]
    spec = np.tile([-2.5, 3.0], (nf, 1))
    spec[nf - 1] = [-0.5, 0.25]                                       # a range of its own for the last field
    rr = np.tile(-2.5 + (np.arange(T) % nbins + 0.5) * (5.5 / nbins), (nf, 1))
    e = np.sort(np.random.default_rng(SEED + nbins).uniform(-2.0, 2.0, size=(nf, nbins + 1)), axis=1)
    if nbins >= 2:
        e[:, nbins // 2] = e[:, nbins // 2 - 1]
    worst = 0.0
    for what, u, sp_, edges, cond in (("normal", d["u"], spec, False, None), ("sorted", d["sorted"], spec, False, None),
                                      ("round-robin", rr, spec, False, None), ("cond", d["u"], spec, False, d["c"]),
                                      ("edges", d["u"], e, True, None), ("edges cond", d["sorted"], e, True, d["c"])):
        r, _ = run_hist(h, dims, nf, d, u, nbins, sp_, edges, cond)
        print("stats-ratio histogram %s nf %d nbins %d %s: %.3g of the bar" % (ids(dims), nf, nbins, what, r))
        assert r <= 1.0, (what, r)
        worst = max(worst, r)
    print("stats-ratio histogram %s nf %d nbins %d: worst %.3g" % (ids(dims), nf, nbins, worst))


@pytest.mark.parametrize("dims,nf", CASES, ids=ids)
def test_histogram_edge_values(dims, nf):
    """A constant field equal to lo (all in bin 0) and one equal to hi (all in overflow); values exactly on the dyadic edges of
    lo = -1, hi = 1, nbins = 64 (value k / 32 - 1 is in bin k; 1.0 in overflow); +-Inf, -0.0 and denormals; a reversed, an
    empty and an infinite range (everything that is not NaN in overflow); a range whose width overflows."""
    d = data(dims, nf)
    h = handle(dims, nf)
    T = d["T"]
    lohi = np.tile([-1.0, 1.0], (nf, 1))
    for v, slot in ((-1.0, 1), (1.0, 64 + 1)):
        r, out = run_hist(h, dims, nf, d, np.full((nf, T), v), 64, lohi)
        assert r <= 1.0 and (out[:, 1, slot] == T).all()
    dy = np.tile(-1.0 + (np.arange(T) % 65) / 32.0, (nf, 1))
    r, out = run_hist(h, dims, nf, d, dy, 64, lohi)
    assert r <= 1.0
    assert (out[:, 1, 1:66] == np.bincount(np.arange(T) % 65, minlength=65)).all() and (out[:, 1, 0] == 0).all()
    sv = np.array([np.inf, -np.inf, -0.0, 0.0, 5e-324, -5e-324, 1e-310, 1.0 - 2.0 ** -53, -1.0 - 2.0 ** -52])
    u = d["u"].copy()
    pos = np.arange(T)[:: max(1, T // 9)][:9]
    u[:, pos] = sv[: len(pos)]
    for nb in (64, 65):
        r, _ = run_hist(h, dims, nf, d, u, nb, lohi)
        assert r <= 1.0
        r, _ = run_hist(h, dims, nf, d, u, nb, np.tile([0.0, 1.0], (nf, 1)))          # -0.0 and -5e-324 on either side of lo = 0
        assert r <= 1.0
    un = d["u"].copy()
    un[0, T // 2] = np.nan
    for bad in ([1.0, -1.0], [0.5, 0.5], [-np.inf, 1.0], [-1.0, np.inf], [np.nan, 1.0]):
        r, out = run_hist(h, dims, nf, d, un, 7, np.tile(bad, (nf, 1)))
        assert r <= 1.0
        assert out[0, 1, 7 + 1] == T - 1 and out[0, 1, 7 + 2] == 1 and (out[1:, 1, 7 + 1] == T).all()
    r, _ = run_hist(h, dims, nf, d, d["u"] * 1e307, 64, np.tile([-1e308, 1e308], (nf, 1)))
    assert r <= 1.0


@pytest.mark.parametrize("dims,nf", CASES, ids=ids)
def test_nan_isolation(dims, nf):
    """A NaN planted at the first, a middle and the last element of one field: every other field keeps its bits, in histogram
    and in summary; within the field only the slot that lost the value and the NaN slot change.  A NaN in `cond`: only the mass
    of its bin becomes NaN."""
    d = data(dims, nf)
    h = handle(dims, nf)
    T = d["T"]
    nb = 64
    spec = np.tile([-2.5, 3.0], (nf, 1))
    sd = dev(spec)
    base = host(h.histogram(dev(d["u"]), nb, range=sd))
    sbase = host(h.summary(dev(d["u"])))
    slots = ref.field_slots(nf, d["u"], nb, spec, False)
    f = nf // 2
    for i in (0, T // 2, T - 1):
        u = d["u"].copy()
        u[f, i] = np.nan
        r, out = run_hist(h, dims, nf, d, u, nb, spec)
        assert r <= 1.0
        other = np.arange(nf) != f
        assert (bits(out[other]) == bits(base[other])).all()
        changed = np.zeros(nb + 3, dtype=bool)
        changed[[slots[f, i], nb + 2]] = True
        assert (bits(out[f][:, ~changed]) == bits(base[f][:, ~changed])).all()
        assert out[f, 1, nb + 2] == 1 and out[f, 1, slots[f, i]] == base[f, 1, slots[f, i]] - 1
        so = host(h.summary(dev(u)))
        assert (bits(so[other]) == bits(sbase[other])).all() and so[f, 4] == 1
        ui = d["u"].copy()
        ui[f, i] = np.inf
        assert (bits(host(h.summary(dev(ui)))[other]) == bits(sbase[other])).all()
        c = d["c"].copy()
        c[f, i] = np.nan
        cbase = host(h.histogram(dev(d["u"]), nb, range=sd, cond=dev(d["c"])))
        r, out = run_hist(h, dims, nf, d, d["u"], nb, spec, cond=c)
        assert r <= 1.0
        keep = np.ones((nf, 2, nb + 3), dtype=bool)
        keep[f, 0, slots[f, i]] = False
        assert (bits(out[keep]) == bits(cbase[keep])).all() and np.isnan(out[f, 0, slots[f, i]])


# ---- 3. cfl ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [c[0] for c in CASES], ids=ids)
def test_cfl(dims):
    """d = 1, 2, 3 and 5; scale == 1 and != 1; N(0, 1); the maximum placed at an end node, at the neighbour of an end node and in
    the middle; a tie (the first index); a NaN in one component, and two of them (the first node).  The value and the index
    equal the double restatement bit for bit, and both are inside the bar against the long-double sums."""
    d = len(dims)
    T = int(np.prod(dims))
    h = handle(dims, [nf for dd, nf in CASES if dd == dims][0])
    rng = np.random.default_rng(SEED + sum(dims))
    vel = rng.standard_normal((d, T))
    strides = [int(np.prod(dims[k + 1:])) for k in range(d)]
    for scale in (None, tuple(2.0 / (1.0 + 0.75 * k) for k in range(d))):
        rs = ref.rates(dims, scale)
        variants = [vel]
        for pos in (0, 1, None, -2, -1):                              # end, neighbour of the end, middle
            idx = sum(((dims[k] // 2 if pos is None else pos % dims[k]) * strides[k]) for k in range(d))
            v = vel.copy()
            v[rng.integers(d), idx] = 1e6 * (1 if pos in (0, None) else -1)
            variants.append(v)
        v = np.zeros((d, T))
        v[0, [T // 3, T - 1 - T // 3]] = 1.0                          # symmetric nodes: equal rates, the first one counts
        variants.append(v)
        variants.append(np.zeros((d, T)))                             # all zero: 0 at index 0
        for v in variants:
            out = host(h.cfl(dev(v), scale))
            want = ref.cfl_restate(dims, rs, v)
            assert (bits(out) == bits(np.array(want))).all(), (out, want)
            assert ref.cfl_ratio(dims, rs, v, out) <= 1.0
        v = vel.copy()
        v[d - 1, T // 2] = np.nan
        out = host(h.cfl(dev(v), scale))
        assert np.isnan(out[0]) and out[1] == T // 2 and ref.cfl_ratio(dims, rs, v, out) == 0.0
        v[0, T - 1] = np.nan
        if T > 2:
            v[0, T // 2 + 1] = np.inf
        out = host(h.cfl(dev(v), scale))
        assert np.isnan(out[0]) and out[1] == T // 2
        out = host(h.cfl(dev(vel), scale))                            # clean data after NaN data
        assert (bits(out) == bits(np.array(ref.cfl_restate(dims, rs, vel)))).all()


# ---- 4. cross-checks against existing modules -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,nf", CASES, ids=ids)
def test_against_integrate(dims, nf):
    """sum of the masses over the slots = integrate(1), M_1 about 0 = integrate(u), M_2 = integrate(u, u), each within the sum of
    the two bars ((T + d + p + 4) U B, or (T_b + d + 3) U B_b summed over the slots, here and (T + 8) U B of ChebModal.integrate, as
    test_gpu_reduce.py takes it); masses with all-ones weights equal the
    counts bit for bit."""
    d = data(dims, nf)
    h = handle(dims, nf)
    T, nd = d["T"], len(dims)
    m = sp.ChebModal(dims, nf)
    u = dev(d["u"])
    one = torch.ones_like(u)
    W = np.abs(ref.node_weights(dims, d["ws"], np.float64).ravel())
    s = host(h.summary(u))
    i1, i2, i0 = host(m.integrate(u)), host(m.integrate(u, u)), host(m.integrate(one))
    B1, B2 = (W * np.abs(d["u"])).sum(axis=1), (W * d["u"] ** 2).sum(axis=1)
    assert (np.abs(s[:, 5] - i1) <= (2 * T + nd + 13) * U * B1).all()
    assert (np.abs(s[:, 6] - i2) <= (2 * T + nd + 14) * U * B2).all()
    spec = dev(np.tile([-2.5, 3.0], (nf, 1)))
    for nb in (64, 1024):
        out = host(h.histogram(u, nb, range=spec))
        tot = out[:, 0].astype(LD).sum(axis=1).astype(np.float64)
        assert (np.abs(tot - i0) <= (2 * T + nd + 11) * U * W.sum()).all()
    for k in range(nd):
        h.set_weights(k, np.ones(dims[k]))
    try:
        for nb in (63, 1024):
            out = host(h.histogram(u, nb, range=spec))
            assert (bits(out[:, 0]) == bits(out[:, 1])).all() and (out[:, 1].sum(axis=1) == T).all()
    finally:
        for k in range(nd):
            h.set_weights(k, None)
    m.destroy()


# ---- 5. repeated calls ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,nf", [((7, 3), 3), ((33, 34, 35), 16), ((96, 97, 95), 1)], ids=ids)
def test_repeats_bit_for_bit(dims, nf):
    """Two calls give equal bits, as does a call on a second stream; a call on clean data after one on NaN data gives the bits
    of a fresh handle."""
    d = data(dims, nf)
    h = handle(dims, nf)
    nd = len(dims)
    u, c = dev(d["u"]), dev(d["c"])
    vel = dev(np.random.default_rng(SEED).standard_normal(nd * d["T"]))
    spec = dev(np.tile([-2.5, 3.0], (nf, 1)))
    e = dev(np.tile(np.linspace(-2.0, 2.0, 257), (nf, 1)))

    def everything(hh):
        return [hh.summary(u), hh.histogram(u, 64, range=spec), hh.histogram(u, 1024, range=spec, cond=c),
                hh.histogram(u, 256, edges=e), hh.cfl(vel)]

    first = [host(x) for x in everything(h)]
    again = [host(x) for x in everything(h)]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        other = everything(h)
    st.synchronize()
    other = [host(x) for x in other]
    bad = d["u"].copy()
    bad[:, ::3] = np.nan
    ub = dev(bad)
    h.summary(ub), h.histogram(ub, 64, range=spec), h.histogram(ub, 1024, range=spec, cond=ub), h.cfl(dev(np.full(nd * d["T"], np.nan)))
    after = [host(x) for x in everything(h)]
    fresh_h = sp.ChebStats(dims, nf, max_bins=1024)
    fresh = [host(x) for x in everything(fresh_h)]
    fresh_h.destroy()
    for a, b, c2, f2, g in zip(first, again, other, after, fresh):
        assert (bits(a) == bits(b)).all() and (bits(a) == bits(c2)).all() and (bits(a) == bits(f2)).all() and (bits(a) == bits(g)).all()


# ---- 6. the interface -----------------------------------------------------------------------------------------------------------
def test_interface_and_wrappers():
    dims, nf = (7, 3), 3
    d = data(dims, nf)
    h = handle(dims, nf)
    u = dev(d["u"])
    s = host(h.summary(u))
    # range=None: auto_range of each field, so nothing under- or overflows and the maximum is in the last bin
    out = host(h.histogram(u, 8))
    assert out.shape == (nf, 2, 11) and (out[:, 1, 0] == 0).all() and (out[:, 1, 9:] == 0).all() and (out[:, 1, 8] >= 1).all()
    spec = np.stack([s[:, 0], s[:, 1] + 2.0 ** -40 * ((s[:, 1] - s[:, 0]) + np.abs(s[:, 1]) + np.abs(s[:, 0]))], axis=1)
    assert (bits(host(h.auto_range(h.summary(u)))) == bits(spec)).all()
    assert (bits(out) == bits(host(h.histogram(u, 8, range=spec)))).all()
    assert (bits(host(h.histogram(u, 8, range=(-1.0, 1.0)))) == bits(host(h.histogram(u, 8, range=np.tile([-1.0, 1.0], (nf, 1)))))).all()
    e = np.linspace(-1.0, 1.0, 9)
    assert (bits(host(h.histogram(u, 8, edges=e))[:, 1]) == bits(host(h.histogram(u, 8, range=(-1.0, 1.0)))[:, 1])).all()
    with pytest.raises(sp.ChebhipError) as err:
        h.histogram(u, 3, edges=[0.0, 1.0, 0.5, 2.0])
    assert err.value.code == 4
    for nb in (0, 1025):
        with pytest.raises(sp.ChebhipError) as err:
            h.histogram(u, nb, range=(-1.0, 1.0))
        assert err.value.code == 4
    with pytest.raises(sp.ChebhipError) as err:
        sp.ChebStats(dims, nf, max_bins=8).histogram(u, 9, range=(-1.0, 1.0))
    assert err.value.code == 4
    with pytest.raises(ValueError):
        h.histogram(u, 8, range=(-1.0, 1.0), edges=e)
    with pytest.raises(AssertionError):
        h.summary(u[:-1])
    with pytest.raises(sp.ChebhipError):
        h.set_weights(2, None)
    # solve.pdf: integrates to 1 over the in-range mass; equals the masses of the histogram over their total and the bin width
    cen, den = solve.pdf(sp, dims, u, 8)
    cen, den = host(cen), host(den)
    width = (spec[:, 1] - spec[:, 0]) / 8
    assert np.allclose((den * width[:, None]).sum(axis=1), 1.0, rtol=1e-14, atol=0)
    assert np.allclose(den, out[:, 0, 1:9] / (out[:, 0, 1:9].sum(axis=1)[:, None] * width[:, None]), rtol=1e-14, atol=0)
    assert np.allclose(cen, spec[:, :1] + (np.arange(8) + 0.5) * width[:, None], rtol=1e-14, atol=1e-300)
    cen, den = solve.pdf(sp, dims, u, 4, range=(10.0, 11.0))
    assert (host(den) == 0).all()
    # solve.cfl_dt
    vel = np.random.default_rng(SEED).standard_normal((2, 21))
    scale = (2.0, 0.5)
    val, idx = ref.cfl_restate(dims, ref.rates(dims, scale), vel)
    dt, at = solve.cfl_dt(sp, dims, dev(vel), cfl=0.4, scale=scale)
    assert dt == 0.4 / val and at == idx
    vel[1, 5] = np.nan
    dt, at = solve.cfl_dt(sp, dims, dev(vel), scale=scale)
    assert dt != dt and at == 5
    assert solve.cfl_dt(sp, dims, dev(np.zeros((2, 21))))[0] == np.inf
