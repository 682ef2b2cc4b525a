"""The truth the cheb_stats_* tests compare against (helper module of test_stats_host.py / test_gpu_stats.py): summary, histogram
and cfl of include/chebhip.h restated in numpy.  What is a sum is formed in long double over the DOUBLE inputs, with W_i the
long-double product of the weights the device is given; what is a decision (the slot of a value, an extremum and its index, a
count) is formed exactly as the header states it, in double.  With U = 2^-53, T values per field, d directions:

    |M_p - truth|  <= (T + d + p + 4) U sum_i |W_i| |u_i - c|^p     d - 1 roundings for W, one for u - c, p - 1 for the power, one
                                                                    for the product, T - 1 additions in any order, a few spare
    |mass - truth| <= (T_b + d + 3) U sum_{i in slot} |W_i c_i|     T_b = the count of the slot; exactly +0.0 for T_b = 0
    cfl: |out - S_idx| <= (d + 2) U S_idx  and  max_i S_i - out <= (d + 2) U max_i S_i,   S_i the long-double sum at node i

`restate_*` are the same quantities in plain double numpy, the stand-in for a device where there is none; their `fault` plants a
mistake that the checks below must catch (test_stats_host.py)."""
import numpy as np

import __graft_entry__ as ge

sp = ge.load()
LD = np.longdouble
U = 2.0 ** -53
SUMMARY = 9


def default_weights(dims):
    return [sp.cc_weights(n) for n in dims]


def node_weights(dims, ws, dtype=LD):
    """W_i = prod_k w_k[i_k] of shape dims, multiplied in ascending k in `dtype`."""
    W = np.asarray(ws[0]).astype(dtype)
    for w in ws[1:]:
        W = np.multiply.outer(W, np.asarray(w).astype(dtype))
    return W.reshape(tuple(dims))


def _ratio(err, bar):
    """The worst err / bar; bar == 0 counts as 0 if err is exactly 0 and as inf otherwise; a NaN counts as inf."""
    err, bar = np.asarray(err, dtype=np.float64), np.asarray(bar, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


# ---- summary --------------------------------------------------------------------------------------------------------------------
def summary_truth(dims, nf, ws, u, center=None):
    """dict: mn, mx (double, the element's bits), imn, imx, nan (exact), M (nf, 4) long double, B (nf, 4) double."""
    T = int(np.prod(dims))
    u = np.asarray(u, dtype=np.float64).reshape(nf, T)
    c = np.zeros(nf) if center is None else np.asarray(center, dtype=np.float64).reshape(nf)
    W = node_weights(dims, ws).ravel()
    mn, mx = np.full(nf, np.inf), np.full(nf, -np.inf)
    imn, imx, nan = np.full(nf, -1.0), np.full(nf, -1.0), np.zeros(nf)
    M, B = np.zeros((nf, 4), dtype=LD), np.zeros((nf, 4))
    for f in range(nf):
        idx = np.flatnonzero(~np.isnan(u[f]))
        nan[f] = T - idx.size
        if idx.size:
            sub = u[f][idx]
            a, b = int(np.argmin(sub)), int(np.argmax(sub))        # the first occurrence; -0.0 == +0.0
            mn[f], mx[f], imn[f], imx[f] = sub[a], sub[b], idx[a], idx[b]
        with np.errstate(invalid="ignore", over="ignore"):
            x = u[f].astype(LD) - LD(c[f])
            xp = np.ones_like(x)
            for p in range(4):
                xp = xp * x
                M[f, p] = (W * xp).sum()
                B[f, p] = float((np.abs(W) * np.abs(xp)).sum())
    return dict(mn=mn, mx=mx, imn=imn, imx=imx, nan=nan, M=M, B=B)


def summary_ratio(dims, nf, out, tr, underflow=False):
    """The worst error / bar over the moments of every field; inf if an exact entry (slots 0..4, bits included) is wrong or a
    moment whose truth is not finite came out finite.  The bar counts relative roundings, which holds for results in the normal
    range only; underflow = True (fields of subnormal values) adds what the number format adds there: an operation whose result
    is subnormal is off by at most one unit 2^-1074, and M_p takes T (p + 2) operations."""
    out = np.asarray(out, dtype=np.float64).reshape(nf, SUMMARY)
    T, d = int(np.prod(dims)), len(dims)
    exact = np.stack([tr["mn"], tr["mx"], tr["imn"], tr["imx"], tr["nan"]], axis=1)
    if not (out[:, :5].view(np.int64) == exact.view(np.int64)).all():
        return np.inf
    worst = 0.0
    for p in range(4):
        t = tr["M"][:, p]
        fin = np.isfinite(t.astype(np.float64)) & np.isfinite(tr["B"][:, p])
        if np.isfinite(out[~fin, 5 + p]).any():
            return np.inf
        err = np.abs(out[fin, 5 + p].astype(LD) - t[fin]).astype(np.float64)
        worst = max(worst, _ratio(err, (T + d + p + 1 + 4) * U * tr["B"][fin, p] + (T * (p + 3) * 2.0 ** -1074 if underflow else 0.0)))
    return worst


def restate_summary(dims, nf, ws, u, center=None, fault=None):
    """(nf, 9) in plain double.  fault: "drop_last" leaves the last element of every field out, "swap_weights" exchanges the
    weights of the first two directions (where their extents allow it: the leading values of each are used)."""
    T = int(np.prod(dims))
    u = np.asarray(u, dtype=np.float64).reshape(nf, T)
    c = np.zeros(nf) if center is None else np.asarray(center, dtype=np.float64).reshape(nf)
    W = node_weights(dims, _swap(dims, ws) if fault == "swap_weights" else ws, np.float64).ravel()
    keep = T - 1 if fault == "drop_last" else T
    out = np.empty((nf, SUMMARY))
    for f in range(nf):
        v = u[f][:keep]
        idx = np.flatnonzero(~np.isnan(v))
        out[f, :5] = [np.inf, -np.inf, -1.0, -1.0, keep - idx.size]
        if idx.size:
            sub = v[idx]
            a, b = int(np.argmin(sub)), int(np.argmax(sub))
            out[f, :4] = [sub[a], sub[b], idx[a], idx[b]]
        with np.errstate(invalid="ignore", over="ignore"):
            x = v - c[f]
            xp = np.ones_like(x)
            for p in range(4):
                xp = xp * x
                out[f, 5 + p] = (W[:keep] * xp).sum()
    return out


def _swap(dims, ws):
    """The weights of directions 0 and 1 exchanged, each cut or repeated to the other's extent."""
    a, b = np.resize(ws[1], dims[0]), np.resize(ws[0], dims[1])
    return [a, b] + list(ws[2:])


# ---- histogram ------------------------------------------------------------------------------------------------------------------
def slots_uniform(u, lo, hi, nbins, fault=None):
    """The slot of every value, CHEB_STATS_UNIFORM, in double as the header states it.  fault "gt": `t > nbins` in place of
    `t >= nbins` with the last bin closed (the convention of numpy.histogram), so a value equal to hi lands in the last bin."""
    u = np.asarray(u, dtype=np.float64)
    lo, hi = np.float64(lo), np.float64(hi)
    s = np.empty(u.shape, dtype=np.int64)
    isn = np.isnan(u)
    s[isn] = nbins + 2
    v = ~isn
    if not (lo < hi and np.isfinite(lo) and np.isfinite(hi)):
        s[v] = nbins + 1
        return s
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        inv = np.float64(nbins) / (hi - lo)
        t = (u - lo) * inv
        under = v & (u < lo)
        if fault == "gt":
            over = v & ~under & ~(t <= np.float64(nbins))
            b = np.minimum(np.floor(np.where(v & ~under & ~over, t, 0.0)).astype(np.int64), nbins - 1)
        else:
            over = v & ~under & ~(t < np.float64(nbins))
            b = np.floor(np.where(v & ~under & ~over, t, 0.0)).astype(np.int64)
    s[v] = 1 + b[v]
    s[under] = 0
    s[over] = nbins + 1
    return s


def slots_edges(u, e, nbins):
    """The slot of every value, CHEB_STATS_EDGES: the last b with e[b] <= u."""
    u, e = np.asarray(u, dtype=np.float64), np.asarray(e, dtype=np.float64)
    assert e.shape == (nbins + 1,)
    isn = np.isnan(u)
    s = np.searchsorted(e, np.where(isn, e[0], u), side="right").astype(np.int64)      # values of e that are <= u
    s = np.where(s == 0, 0, np.where(u >= e[nbins], nbins + 1, s))
    s[isn] = nbins + 2
    return s


def slots_brute(u, nbins, lo=None, hi=None, e=None):
    """One value at a time, in Python floats: the loop the two functions above are tested against."""
    out = []
    for x in np.asarray(u, dtype=np.float64).tolist():
        if x != x:
            out.append(nbins + 2)
        elif e is not None:
            if x < e[0]:
                out.append(0)
            elif x >= e[nbins]:
                out.append(nbins + 1)
            else:
                out.append(1 + max(b for b in range(nbins) if e[b] <= x))
        elif not (lo < hi and abs(lo) < float("inf") and abs(hi) < float("inf")):
            out.append(nbins + 1)
        elif x < lo:
            out.append(0)
        else:
            t = (x - lo) * (float(nbins) / (hi - lo))
            out.append(1 + int(t) if t < nbins else nbins + 1)
    return np.array(out, dtype=np.int64)


def field_slots(nf, u, nbins, spec, edges):
    """(nf, T) slots; spec: (nf, 2) bounds or (nf, nbins + 1) edges."""
    u = np.asarray(u, dtype=np.float64).reshape(nf, -1)
    spec = np.asarray(spec, dtype=np.float64).reshape(nf, -1)
    return np.stack([slots_edges(u[f], spec[f], nbins) if edges else slots_uniform(u[f], spec[f, 0], spec[f, 1], nbins)
                     for f in range(nf)])


def _sorter(slots, nslots):
    """(order, starts, nonempty) of a stable sort of the values by slot."""
    order = np.argsort(slots, kind="stable")
    ss = slots[order]
    starts = np.searchsorted(ss, np.arange(nslots), side="left")
    return order, starts, np.searchsorted(ss, np.arange(nslots), side="right") > starts


def _slot_sums(terms, sorter):
    """The sum of terms per slot, in the dtype of terms (one reduceat over the sorted terms)."""
    order, starts, nonempty = sorter
    tt = terms[order]
    with np.errstate(invalid="ignore", over="ignore"):
        red = np.add.reduceat(np.append(tt, tt.dtype.type(0)), starts)       # starts <= size: the appended 0 ends the last range
    return np.where(nonempty, red, np.zeros(starts.size, dtype=terms.dtype))


def histogram_truth(dims, nf, ws, slots, nbins, cond=None):
    """dict: mass (nf, nbins + 3) long double, B the same in double, count (exact)."""
    T = int(np.prod(dims))
    W = node_weights(dims, ws).ravel()
    ns = nbins + 3
    mass, B, cnt = np.zeros((nf, ns), dtype=LD), np.zeros((nf, ns)), np.zeros((nf, ns))
    c = None if cond is None else np.asarray(cond, dtype=np.float64).reshape(nf, T)
    for f in range(nf):
        with np.errstate(invalid="ignore", over="ignore"):
            terms = W if c is None else W * c[f].astype(LD)
            srt = _sorter(slots[f], ns)
            mass[f] = _slot_sums(terms, srt)
            B[f] = _slot_sums(np.abs(terms), srt).astype(np.float64)
        cnt[f] = np.bincount(slots[f], minlength=ns)
    return dict(mass=mass, B=B, count=cnt)


def histogram_ratio(dims, nf, nbins, out, tr):
    """The worst error / bar over every slot of every field; inf if a count is wrong, the counts of a field do not sum to T, an
    empty slot's mass is not +0.0, or a mass whose truth is not finite came out finite."""
    ns, d, T = nbins + 3, len(dims), int(np.prod(dims))
    out = np.asarray(out, dtype=np.float64).reshape(nf, 2, ns)
    if not (out[:, 1] == tr["count"]).all() or not (out[:, 1].sum(axis=1) == T).all():
        return np.inf
    empty = tr["count"] == 0
    if not (out[:, 0][empty].view(np.int64) == 0).all():
        return np.inf
    t = tr["mass"]
    fin = np.isfinite(t.astype(np.float64)) & np.isfinite(tr["B"]) & ~empty
    if np.isfinite(out[:, 0][~fin & ~empty]).any():
        return np.inf
    err = np.abs(out[:, 0][fin].astype(LD) - t[fin]).astype(np.float64)
    return _ratio(err, (tr["count"][fin] + d + 3) * U * tr["B"][fin])


def restate_histogram(dims, nf, ws, u, nbins, spec, edges=False, cond=None, fault=None):
    """(nf, 2, nbins + 3) in plain double (numpy.bincount with weights).  fault: "gt" (see slots_uniform), "drop_last",
    "swap_weights"."""
    T = int(np.prod(dims))
    u = np.asarray(u, dtype=np.float64).reshape(nf, T)
    spec = np.asarray(spec, dtype=np.float64).reshape(nf, -1)
    W = node_weights(dims, _swap(dims, ws) if fault == "swap_weights" else ws, np.float64).ravel()
    c = None if cond is None else np.asarray(cond, dtype=np.float64).reshape(nf, T)
    keep = T - 1 if fault == "drop_last" else T
    out = np.zeros((nf, 2, nbins + 3))
    for f in range(nf):
        s = slots_edges(u[f], spec[f], nbins) if edges else slots_uniform(u[f], spec[f, 0], spec[f, 1], nbins,
                                                                          "gt" if fault == "gt" else None)
        terms = W if c is None else W * c[f]
        out[f, 0] = np.bincount(s[:keep], weights=terms[:keep], minlength=nbins + 3)
        out[f, 1] = np.bincount(s[:keep], minlength=nbins + 3)
    return out


# ---- cfl ------------------------------------------------------------------------------------------------------------------------
def spacing_ld(n):
    """h_j in long double: the gap between the nodes j and j + 1 is 2 sin(pi (2j + 1) / 2N) sin(pi / 2N)."""
    N = n - 1
    pi = LD(4) * np.arctan(LD(1))
    j = np.arange(N)
    gap = LD(2) * np.sin(pi * (2 * j + 1).astype(LD) / LD(2 * N)) * np.sin(pi / LD(2 * N))
    h = np.empty(n, dtype=LD)
    h[0], h[N] = gap[0], gap[N - 1]
    if n > 2:
        h[1:N] = np.minimum(gap[:-1], gap[1:])
    return h


def rates(dims, scale=None):
    """The r_k the device is given (cheb_stats_rate_host)."""
    return [sp.stats_rate(n, 1.0 if scale is None else scale[k]) for k, n in enumerate(dims)]


def cfl_sums(dims, rs, vel, dtype=LD):
    """S_i = sum_k |vel_k(i)| r_k[i_k] of shape dims: products and sums in `dtype`, k ascending."""
    d = len(dims)
    v = np.asarray(vel, dtype=np.float64).reshape((d,) + tuple(dims))
    S = None
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(d):
            shape = [1] * d
            shape[k] = dims[k]
            term = np.abs(v[k]).astype(dtype) * np.asarray(rs[k]).astype(dtype).reshape(shape)
            S = term if S is None else S + term
    return S


def cfl_restate(dims, rs, vel, fault=None):
    """(value, index) in plain double, every product rounded and added in ascending k: what the device computes, bit for bit.
    A NaN anywhere: (NaN, the first such node).  fault: "drop_last"."""
    S = cfl_sums(dims, rs, vel, np.float64).ravel()
    if fault == "drop_last":
        S = S[:-1]
    isn = np.isnan(S)
    if isn.any():
        return np.nan, float(np.flatnonzero(isn)[0])
    i = int(np.argmax(S))
    return float(S[i]), float(i)


def cfl_ratio(dims, rs, vel, out):
    """The worst of |out - S_idx| / ((d + 2) U S_idx) and (max S - out) / ((d + 2) U max S); for data with a NaN: 0 if out is
    (NaN, the first node with a NaN), inf otherwise."""
    d = len(dims)
    val, idx = float(out[0]), float(out[1])
    S = cfl_sums(dims, rs, vel).ravel()
    isn = np.isnan(S.astype(np.float64))
    if isn.any():
        return 0.0 if (val != val and idx == np.flatnonzero(isn)[0]) else np.inf
    if not (0 <= idx < S.size and idx == int(idx)) or val != val:
        return np.inf
    at, top = S[int(idx)], S.max()
    return max(_ratio([float(abs(LD(val) - at))], [(d + 2) * U * float(at)]),
               _ratio([max(float(top - LD(val)), 0.0)], [(d + 2) * U * float(top)]))
