"""Newton-Krylov driver on device vectors: the roles of SNESSolve and KSPSolve(KSPFGMRES) around the elliptic
callbacks (elliptic.C:177-185, 213), for end-to-end solves where no PETSc exists.

Each Newton step evaluates FormFunction (which leaves eta, eta', grad u behind, elliptic.C:498-509), then
solves J dx = -F with the matrix-free Jacobian MatMult_Elliptic (elliptic.C:297-339) by restarted FGMRES
(chebhip_fgmres_*), and updates x along dx with a backtracking line search; `M` is the slot for a right preconditioner
(the reference uses ILU(2) of a finite-difference matrix, elliptic.C:184-185, which stays PETSc's).
poisson_solve is the direct route for the linear problem (gamma = 0): one FormFunction and one fast-diagonalisation solve.
"""
import torch


def newton_krylov(sp, op, b, x, gamma=0.0, exponent=2.0, snes_rtol=1e-8, snes_atol=1e-50, snes_max_it=50,
                  ksp_rtol=1e-5, ksp_restart=30, ksp_max_it=10000, M=None, monitor=None, norm=None, line_search=True, ks=None):
    """Solve FormFunction(x) = A(x) x - b = 0 in place in x (device tensor).  Returns (newton_its, total_ksp_its, |F|).
    On several ranks (vectors = this rank's pieces) `op` is a callable driver of dist.py, `sp.Fgmres` must return a
    solver with its reduction set, and `norm` the global 2-norm.
    ks: a caller's Fgmres to use and keep (as a KSP object outlives its solves, elliptic.C:181-185); None: one is made and destroyed here."""
    n = op.global_size
    norm = norm or (lambda t: float(t.norm()))
    F = torch.empty_like(x)
    dx = torch.empty_like(x)
    own_ks = ks is None
    if own_ks:
        ks = sp.Fgmres(n, restart=ksp_restart, rtol=ksp_rtol, max_it=ksp_max_it)
    total = 0
    op.function(x, b, F, gamma, exponent)
    f0 = fn = norm(F)
    it = 0
    try:
        while it < snes_max_it and fn > max(snes_rtol * f0, snes_atol):
            F.neg_()
            ks.solve(op, F, dx, M=M)                    # J dx = -F, state of the last FormFunction
            total += ks.iterations
            if ks.reason < 0:                           # KSP_DIVERGED_*: SNES stops with SNES_DIVERGED_LINEAR_SOLVE
                raise RuntimeError("Newton step %d: linear solve diverged (reason %d after %d iterations, residual %.3e)"
                                   % (it + 1, ks.reason, ks.iterations, ks.residual))
            # backtracking line search on |F| (the role of SNES's default line search, elliptic.C:177-179:
            # SNESCreate leaves SNESLS in place): full step first, halved until sufficient decrease
            lam, fold = 1.0, fn
            x.add_(dx)
            op.function(x, b, F, gamma, exponent)
            fn = norm(F)
            while line_search and not (fn <= (1.0 - 1e-4 * lam) * fold) and lam > 1e-6:
                x.add_(dx, alpha=-0.5 * lam)
                lam *= 0.5
                op.function(x, b, F, gamma, exponent)
                fn = norm(F)
            it += 1
            if monitor:
                monitor(it, fn, ks.iterations)
    finally:
        if own_ks:
            ks.destroy()
    return it, total, fn


def poisson_solve(sp, op, b, x, sigma=0.0, solver=None):
    """The linear problem sigma u + A u = b with the Dirichlet values set on `op` (A: MatMult_Elliptic at gamma = 0, eta == 1),
    solved directly instead of by Newton-Krylov: one FormFunction at x = 0 gives F0 = A_IB g - b (the boundary values' part of the
    operator minus the right-hand side), and x = (sigma I + A_II)^-1 (-F0) by fast diagonalisation (sp.HelmholtzSolver).
    b, x: device tensors of op.global_size (x is overwritten; it may not be b).  solver: a caller's HelmholtzSolver(op.dims, sigma)
    to use and keep; None: one is made and destroyed here.  Returns x."""
    own = solver is None
    if own:
        solver = sp.HelmholtzSolver(op.dims, sigma)
    elif solver.dims != tuple(op.dims) or solver.sigma != float(sigma) or solver.size != op.global_size:
        raise ValueError("solver: a HelmholtzSolver of the operator's grid with sigma = %g and one field" % sigma)
    try:
        x.zero_()
        F = torch.empty_like(x)
        op.function(x, b, F, 0.0, 2.0)
        F.neg_()
        solver.solve(F, x)
    finally:
        if own:
            solver.destroy()
    return x


def channel_poisson(sp, dims, f, periodic, scale=None):
    """-sum_k scale_k^2 d_k^2 u = f on a box whose flagged directions are periodic and whose other faces carry u = 0, solved
    directly for the one-off case (a HelmholtzSolver with bc "periodic" / "dirichlet" made and destroyed here).  f: full-grid
    device tensor of prod(dims) values, the nodes fourier_nodes(dims[k]) along a periodic direction and cgl_nodes(dims[k]) along a
    wall one; its wall entries are ignored.  With every direction periodic the problem is singular: the components of f along the
    dropped modes (HelmholtzSolver's docstring) are ignored and u has none.  Returns the full-grid u (a new tensor)."""
    dims = tuple(int(d) for d in dims)
    flags = tuple(bool(p) for p in periodic)
    if len(flags) != len(dims):
        raise ValueError("periodic: expected %d flags, got %d" % (len(dims), len(flags)))
    return helmholtz_bvp(sp, dims, f, None, ["periodic" if p else "dirichlet" for p in flags], 0.0, scale=scale)


def channel_project(sp, dims, u, periodic, scale=None, flux=None):
    """The divergence-free projection of u (nvec * d full-grid fields) on a box whose flagged directions are periodic and whose
    other faces are walls with the outward normal velocity `flux` (None: 0), for the one-off case: project_velocity with bc
    "periodic" / "wall", next to channel_poisson.  The nodes are fourier_nodes(dims[k]) along a periodic direction and
    cgl_nodes(dims[k]) along a wall one.  With every direction periodic there is no wall and flux must be None.  Returns
    (out, phi) (new tensors)."""
    dims = tuple(int(d) for d in dims)
    flags = tuple(bool(p) for p in periodic)
    if len(flags) != len(dims):
        raise ValueError("periodic: expected %d flags, got %d" % (len(dims), len(flags)))
    return project_velocity(sp, dims, u, ["periodic" if p else "wall" for p in flags], scale, flux)


def helmholtz_bvp(sp, dims, f_full, g, bc, sigma=0.0, solver=None, scale=None):
    """sigma u - Laplace u = f with alpha u + beta du/dnu = g on every face (sp.HelmholtzSolver's `bc`), solved directly.
    f_full: full-grid device tensor (its boundary entries are ignored); g: the compact boundary values in row-major node order
    (the ell_op_set_dirichlet layout) or None for zero data.  solver: a caller's HelmholtzSolver(dims, sigma, bc=bc) to use and
    keep (its nfields stacked fields); None: one is made and destroyed here.  scale (None: the cube): the box solve of
    HelmholtzSolver(scale=...), sigma u - sum_k scale_k^2 d_k^2 u = f.  Returns the full-grid u (a new tensor)."""
    dims = tuple(int(d) for d in dims)
    own = solver is None
    if own:
        solver = sp.HelmholtzSolver(dims, sigma, bc=bc, scale=scale)
    elif solver.scale != (None if scale is None else tuple(float(v) for v in scale)):
        raise ValueError("solver: a HelmholtzSolver with the same scale")
    elif solver.dims != dims or solver.sigma != float(sigma) or solver.bc is None or solver.bc != sp.bc_split(bc, len(dims))[2]:
        raise ValueError("solver: a HelmholtzSolver of the grid with sigma = %g and the same bc" % sigma)
    try:
        if f_full.numel() != solver.full_size:
            raise ValueError("f_full has %d elements, expected %d" % (f_full.numel(), solver.full_size))
        inner = tuple(slice(None) if p else slice(1, -1) for p in solver.periodic)      # a periodic direction has no end nodes
        f = f_full.reshape((solver.nfields,) + dims)[(slice(None),) + inner].contiguous().reshape(-1)
        u = torch.empty_like(f_full).contiguous()
        solver.solve_full(f, g, u)
    finally:
        if own:
            solver.destroy()
    return u


def variable_diffusion(sp, dims, kappa, f_full, c=0.0, bc=None, g=None, scale=None, rtol=1e-8, max_it=200, restart=30, singular="refuse",
                       tensor=None, velocity=None):
    """c u - sum_k scale_k^2 d_k(kappa d_k u) = f with alpha u + beta scale_k du/dnu = g on every face (sp.VarHelmholtz's `bc`;
    None: Dirichlet everywhere), by preconditioned FGMRES in one library call.  kappa: a full-grid device tensor (> 0); c: a scalar
    or a full-grid device tensor (>= 0); f_full: the full-grid right-hand side (its boundary entries are ignored; a multiple of the
    grid's size stacks fields); g: the compact boundary values or None.  The faces' conditions do not contain kappa: for Neumann
    data of the flux kappa du/dnu divide g by kappa first.  Returns (u, iterations): the full-grid u (a new tensor) and the
    operator applications of the solve; a solve that does not converge raises RuntimeError.  singular: "refuse" -- a singular
    problem (c == 0, every direction periodic or Neumann / Neumann) raises ChebhipError -- or "deflate": VarHelmholtz.solve_deflated,
    the solution without null-space part of the problem whose source has lost its null-space part.
    tensor, velocity (2-D and 3-D): c u + velocity . grad u - div(K grad u) = f by VarHelmholtz.set_tensor -- tensor: the
    d (d + 1) / 2 full-grid fields of K stacked in the order sp.tensor_order(d), kappa is then not read (None will do); tensor None
    with a velocity: K = kappa I; velocity: d stacked full-grid fields or None.  Scales enter as in the operator: every derivative
    is scale_k d_k."""
    if singular not in ("refuse", "deflate"):
        raise ValueError("singular = %r: 'refuse' or 'deflate'" % (singular,))
    dims = tuple(int(d) for d in dims)
    N = 1
    for n in dims:
        N *= n
    if f_full.numel() == 0 or f_full.numel() % N:
        raise ValueError("f_full has %d elements, no multiple of %d" % (f_full.numel(), N))
    op = sp.VarHelmholtz(dims, f_full.numel() // N, bc=bc, scale=scale)
    try:
        cc = c.contiguous().reshape(-1) if isinstance(c, torch.Tensor) else c
        if tensor is None and velocity is None:
            op.set_coefficients(kappa.contiguous().reshape(-1), cc)
        else:
            if tensor is None:
                k = kappa.contiguous().reshape(-1)
                tensor = torch.cat([k] * len(dims) + [torch.zeros_like(k)] * (len(dims) * (len(dims) - 1) // 2))
            op.set_tensor(tensor.contiguous().reshape(-1), cc, None if velocity is None else velocity.contiguous().reshape(-1))
        inner = tuple(slice(None) if p else slice(1, -1) for p in op.periodic)
        f = f_full.reshape((op.nfields,) + dims)[(slice(None),) + inner].contiguous().reshape(-1)
        u = torch.empty(op.full_size, dtype=torch.float64, device=f_full.device)
        (op.solve_deflated if singular == "deflate" else op.solve)(f, g, u_full=u, rtol=rtol, max_it=max_it, restart=restart)
        if op.reason <= 0:
            raise RuntimeError("variable_diffusion: FGMRES stopped with reason %d after %d iterations (residual %.3e)"
                               % (op.reason, op.iterations, op.residual_norm))
        return u.reshape(f_full.shape), op.iterations
    finally:
        op.destroy()


def project_velocity(sp, dims, u, bc=None, scale=None, flux=None, inverse_density=None, **solve_options):
    """(out, phi) of sp.ChebProject(dims, nvec, bc, scale).project(u, flux=flux) with a handle made and destroyed here: u holds
    nvec * d full-grid fields, out its divergence-free projection (new tensors).  A bc entry "periodic" makes that direction periodic
    (ChebProject's docstring).  inverse_density: kappa = 1 / rho at every node -- the variable-density projection
    out_k = u_k - kappa scale_k d_k phi (ChebProject(variable=True); solve_options: its rtol, atol, max_it, restart); a solve that
    does not converge raises RuntimeError."""
    dims = tuple(int(d) for d in dims)
    N = 1
    for n in dims:
        N *= n
    per = N * len(dims)
    if u.numel() == 0 or u.numel() % per:
        raise ValueError("u has %d elements, no multiple of %d" % (u.numel(), per))
    if inverse_density is None and solve_options:
        raise ValueError("%s: options of the variable-density solve, but no inverse_density" % ", ".join(sorted(solve_options)))
    h = sp.ChebProject(dims, u.numel() // per, bc, scale) if inverse_density is None else sp.ChebProject(dims, u.numel() // per, bc, scale, variable=True)
    try:
        phi = torch.empty((h.nvec,) + dims, dtype=torch.float64, device=u.device)
        if inverse_density is None:
            out = h.project(u, phi=phi, flux=flux)
        else:
            h.set_inverse_density(inverse_density.contiguous().reshape(-1))
            out = h.project(u, phi=phi, flux=flux, **solve_options)
            if h.reason <= 0:
                raise RuntimeError("project_velocity: FGMRES stopped with reason %d after %d iterations (residual %.3e)"
                                   % (h.reason, h.iterations, h.residual_norm))
    finally:
        h.destroy()
    return out, phi


def diffuse(sp, dims, u_full, t, bc, g=None, f=None, kappa=1.0, scale=None):
    """The exact solution at time t of u_t = kappa sum_k scale_k^2 d_k^2 u + f from the full-grid field u_full, with the steady
    conditions alpha u + beta du/dnu = g of `bc` (sp.HelmholtzSolver's) on the faces: u_s + extend(e^(-t kappa A) (u_0 - u_s)_I),
    u_s the steady solution (one HelmholtzSolver.solve_full; 0 without f and g), the exponential one sp.ChebOpFun.apply_full.
    f: full-grid device tensor (boundary entries ignored) or None; g: compact boundary values or None.  u_full is expected to
    meet the conditions; its boundary entries are not read.  Neumann on every face is singular: only f = None, g = None is
    handled there.  No time stepping: any t >= 0 in one call.  Returns a new (*dims) tensor.  A bc entry "periodic" makes that
    direction periodic (nodes fourier_nodes(dims[k]), no faces, no entries in g); every direction periodic or Neumann / Neumann is
    singular in the same sense."""
    dims = tuple(int(n) for n in dims)
    t, kappa = float(t), float(kappa)
    if not (t >= 0.0 and kappa > 0.0):
        raise ValueError("diffuse: t >= 0 and kappa > 0")
    fun = sp.ChebOpFun(dims, 1, 1, 0.0, bc=bc, scale=scale)
    solver = None
    try:
        if u_full.numel() != fun.full_size:
            raise ValueError("u_full has %d elements, expected %d" % (u_full.numel(), fun.full_size))
        steady = f is not None or g is not None
        if steady and fun.singular:
            raise ValueError("diffuse: Neumann conditions on every face have no steady state for general f and g; pass f = None, g = None")
        if any(fun.periodic):                           # the unknowns: every node of a periodic direction, the interior of a wall one
            inner = (slice(None),) + tuple(slice(None) if p else slice(1, -1) for p in fun.periodic)
            pack = lambda x, xi: xi.copy_(x[inner].reshape(-1))
        else:
            pack = lambda x, xi: _layout(sp, dims, u_full.device).pack(1, x, xi=xi)
        v = u_full.reshape((1,) + dims)
        us = None
        if steady:
            solver = sp.HelmholtzSolver(dims, 0.0, bc=bc, scale=scale)
            rhs = torch.zeros(fun.size, dtype=torch.float64, device=u_full.device)
            if f is not None:
                if f.numel() != fun.full_size:
                    raise ValueError("f has %d elements, expected %d" % (f.numel(), fun.full_size))
                pack((f.reshape((1,) + dims) / kappa).contiguous(), rhs)
            us = torch.empty((1,) + dims, dtype=torch.float64, device=u_full.device)
            solver.solve_full(rhs, g, us.reshape(-1))
            v = v - us
        vi = torch.empty(fun.size, dtype=torch.float64, device=u_full.device)
        pack(v.contiguous(), vi)
        fun.set_terms("exp", tau=t * kappa)
        out = fun.apply_full(vi).reshape((1,) + dims)
        if us is not None:
            out += us
        torch.cuda.current_stream().synchronize()       # (the handles' buffers are freed below)
    finally:
        fun.destroy()
        if solver is not None:
            solver.destroy()
    return out[0]


def continuation_schedule(exponent, regularization, cont0=0, cont=1):
    """The (exponent, regularization) pairs of the Newton continuation loop, stokes.C:217-221:
    exponent_i = 1 + (i/cont)^0.8 (exponent - 1), regularization_i = exp(log(regularization) i/cont)."""
    import math
    out = []
    for i in range(cont0, cont + 1):
        out.append((1.0 + math.pow(1.0 * i / cont, 0.8) * (exponent - 1.0), math.exp(math.log(regularization) * i / cont)))
    return out


def stokes_solve(sp, op, x, rheology=(0, 1.0, 1.0, 1.0, 1.0), cont0=0, cont=1, saddle_type=0,
                 snes_rtol=1e-8, snes_atol=1e-50, snes_max_it=50, ksp_rtol=1e-5, ksp_restart=30, ksp_max_it=10000,
                 vel=(4, 1e-5), schur=(3, 1e-5), svel=(0, 1e-5), pc_sweeps=0, line_search=True, monitor=None, max_linear_fail=1,
                 schur_jacobi=True, stats=None, dist=None, ks=None, pc=None):
    """The solve phase of stokes.C:213-235 on device vectors: for every continuation stage, SNESSolve = Newton with a
    backtracking line search around StokesFunction (stokes.C:680-758), each step KSPSolve(KSPFGMRES) on the
    Newton-linearised StokesMatMult (stokes.C:499-519) right-preconditioned by StokesPCApply<saddle_type>
    (stokes.C:1714-1817; MatVVPC re-assembled per step as StokesPCSetUp0 does).  Dirichlet values and force must be
    set on `op`; x (device tensor, global_size) holds the initial guess and the result.
    `max_linear_fail`: linear solves that may end on their iteration limit before the Newton iteration gives up
    (-snes_max_linear_solve_fail, PETSc's default 1); the step of such a solve is still tried by the line search.
    `stats` (a dict) receives "linear_fails": the number of linear solves that ended on their iteration limit.
    `dist`: a slab driver of dist.py (DistStokesC) whose slab-mode operator `op` is: the vectors are this rank's pieces, every
    rank calls collectively; norms, the Krylov inner products and the block preconditioner's sums go through its communicator.
    ks, pc: the caller's outer Fgmres and block preconditioner to use and keep (the KSP / PC objects of stokes.C:155-176 outlive their
    solves); None: made and destroyed here.
    Returns a list of (exponent, regularization, newton_its, ksp_its, |F|) per stage."""
    kind, hardness, exponent, regularization, gamma0 = rheology
    n = op.global_size
    own_ks, own_pc = ks is None, pc is None
    if own_ks:
        ks = sp.Fgmres(n, restart=ksp_restart, rtol=ksp_rtol, max_it=ksp_max_it)
    if dist is not None:
        if own_ks:
            ks.set_reduce_raw(*dist.comm.reduce_fn())
        if own_pc:
            pc = dist.saddle(saddle_type, vel, schur, svel, schur_jacobi)
        gnorm = dist.comm.norm
    else:
        if own_pc:
            pc = sp.StokesSaddlePc(op, saddle_type, vel, schur, svel, pc_sweeps, schur_jacobi)
        gnorm = lambda t: float(t.norm())
    stages = continuation_schedule(exponent, regularization, cont0, cont) if kind == 1 else [(exponent, regularization)]
    fails = [0]
    try:
        out = _stokes_stages(op, x, stages, kind, hardness, gamma0, ks, pc, gnorm, fails, snes_rtol, snes_atol, snes_max_it,
                             line_search, monitor, max_linear_fail)
    finally:
        if own_ks:
            ks.destroy()
        if own_pc:
            pc.destroy()
        if stats is not None:
            stats["linear_fails"] = fails[0]
    return out


def _stokes_stages(op, x, stages, kind, hardness, gamma0, ks, pc, gnorm, fails, snes_rtol, snes_atol, snes_max_it, line_search,
                   monitor, max_linear_fail):
    """The continuation stages `stages` ((exponent, regularization) pairs) of stokes_solve on one grid, x in place; fails[0] counts
    the linear solves that ended on their iteration limit (over all calls that share the list)."""
    F = torch.empty_like(x); dx = torch.empty_like(x)
    out = []
    for (e_i, r_i) in stages:
        op.set_rheology(kind, hardness, e_i, r_i, gamma0)                  # stokes.C:219-220
        op.function(x, F)
        f0 = fn = gnorm(F); it = 0; total = 0
        while it < snes_max_it and fn > max(snes_rtol * f0, snes_atol):
            pc.setup()                                                      # StokesPCSetUp0 after the new viscosity
            F.neg_()
            ks.solve(op, F, dx, M=pc)
            total += ks.iterations
            if ks.reason < 0:
                fails[0] += 1
                if fails[0] >= max_linear_fail or ks.reason != -3:
                    raise RuntimeError("stage (%g, %g) Newton step %d: linear solve diverged (reason %d, %d its, residual %.3e)"
                                       % (e_i, r_i, it + 1, ks.reason, ks.iterations, ks.residual))
            lam, fold = 1.0, fn
            x.add_(dx)
            op.function(x, F); fn = gnorm(F)
            while line_search and not (fn <= (1.0 - 1e-4 * lam) * fold) and lam > 1e-6:
                x.add_(dx, alpha=-0.5 * lam); lam *= 0.5
                op.function(x, F); fn = gnorm(F)
            it += 1
            if monitor:
                monitor(e_i, r_i, it, fn, ks.iterations, lam)
        out.append((e_i, r_i, it, total, fn))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Grid sequencing (PETSc's -snes_grid_sequence): solve on a coarse Chebyshev grid, interpolate the solution to the next grid
# (cheb_resample_*) and use it there as the Newton starting point.  One GPU, no slab distribution.
# ---------------------------------------------------------------------------------------------------------------------------------

_prolong_cache = {}


def _node_split(dims, device):
    """Row-major (BlockIt) indices of the interior and of the boundary nodes of the full grid `dims`, as device index tensors."""
    inside = torch.zeros(tuple(dims), dtype=torch.bool)
    inside[tuple(slice(1, n - 1) for n in dims)] = True
    inside = inside.ravel()
    return torch.nonzero(inside).ravel().to(device), torch.nonzero(~inside).ravel().to(device)


def _prolongation(sp, kind, dims_c, dims_f, device):
    """Index tensors and resamplers of one level pair, built once: (interior, boundary, velocity / scalar resampler, pressure resampler)."""
    dims_c, dims_f = tuple(int(n) for n in dims_c), tuple(int(n) for n in dims_f)
    key = (kind, dims_c, dims_f, str(device))
    if key not in _prolong_cache:
        inner, bnd = _node_split(dims_c, device)
        ncomp = len(dims_c) if kind == "stokes" else 1
        rv = sp.Resample(dims_c, dims_f, "all", "interior", ncomp=ncomp)
        rp = sp.Resample(dims_c, dims_f, "interior", "interior") if kind == "stokes" else None
        _prolong_cache[key] = (inner, bnd, rv, rp)
    return _prolong_cache[key]


def _dev_values(v, like):
    return torch.as_tensor(v, dtype=torch.float64).to(like.device)


def prolong_elliptic(sp, dims_c, x_c, dirichlet_c, dims_f):
    """The global vector of the grid dims_f interpolated from the coarse global vector x_c (interior nodes, row-major) and the
    coarse compact Dirichlet values (ell_op_set_dirichlet order): the full coarse field, resampled ALL -> INTERIOR.  Device tensors
    throughout (dirichlet_c may be a host array)."""
    inner, bnd, r, _ = _prolongation(sp, "elliptic", dims_c, dims_f, x_c.device)
    full = torch.empty(r.size(0), dtype=torch.float64, device=x_c.device)
    full[inner] = x_c
    full[bnd] = _dev_values(dirichlet_c, x_c)
    return r.apply(full, torch.empty(r.size(1), dtype=torch.float64, device=x_c.device))


def prolong_stokes(sp, dims_c, x_c, dirichlet_c, dims_f):
    """The same for a Stokes state [v_0 .. v_{d-1}, p] per interior node: the velocity as the full coarse field with its Dirichlet
    values (node-major, d components) resampled ALL -> INTERIOR, the pressure INTERIOR -> INTERIOR, interleaved again."""
    d = len(dims_c)
    inner, bnd, rv, rp = _prolongation(sp, "stokes", dims_c, dims_f, x_c.device)
    xc = x_c.view(-1, d + 1)
    full = torch.empty((rv.size(0) // d, d), dtype=torch.float64, device=x_c.device)
    full[inner] = xc[:, :d]
    full[bnd] = _dev_values(dirichlet_c, x_c).view(-1, d)
    v = rv.apply(full.view(-1), torch.empty(rv.size(1), dtype=torch.float64, device=x_c.device))
    p = rp.apply(xc[:, d].contiguous(), torch.empty(rp.size(1), dtype=torch.float64, device=x_c.device))
    out = torch.empty((rp.size(1), d + 1), dtype=torch.float64, device=x_c.device)
    out[:, :d] = v.view(-1, d)
    out[:, d] = p
    return out.view(-1)


def newton_krylov_sequenced(sp, levels, gamma=0.0, exponent=2.0, x=None, x0=None, ks=None, monitor=None, dist=None, **newton_kw):
    """Grid-sequenced newton_krylov: levels = [(op, b, dirichlet, M), ...] coarsest first (op an EllipticOp whose Dirichlet values
    are `dirichlet`, b its right-hand side, M its preconditioner or None).  Every level is solved to the tolerances of newton_kw,
    the finer ones from the prolongation of the previous level's solution (PETSc's semantics).
    x: a device tensor of the finest level's global size that receives the solution; x0: the coarsest level's starting point
    (None: zero).  ks: one Fgmres per level to use and keep, or None.  monitor(level, it, |F|, ksp_its) after every
    Newton step.  Returns the per-level (newton_its, ksp_its, |F|)."""
    if dist is not None:
        raise ValueError("grid sequencing runs on one GPU: no slab-distributed levels")
    if x is None or x.numel() != levels[-1][0].global_size:
        raise ValueError("x: a device tensor of the finest level's global size receives the solution")
    out = []
    prev = None
    for lev, (op, b, dirichlet, M) in enumerate(levels):
        n = op.global_size
        last = lev == len(levels) - 1
        if prev is None:
            xl = torch.zeros(n, dtype=torch.float64, device=x.device) if x0 is None else x0.clone()
        else:
            xl = prolong_elliptic(sp, prev[0].dims, prev[1], prev[2], op.dims)
        if last:
            x.copy_(xl); xl = x
        mon = None if monitor is None else (lambda it, fn, k, lev=lev: monitor(lev, it, fn, k))
        out.append(newton_krylov(sp, op, b, xl, gamma, exponent, M=M, monitor=mon, ks=None if ks is None else ks[lev], **newton_kw))
        prev = (op, xl, dirichlet)
    return out


def default_stage_level(nstages, nlevels):
    """Every continuation stage but the last on the coarsest level, the last one on the finest."""
    return [0] * (nstages - 1) + [nlevels - 1]


def stokes_solve_sequenced(sp, levels, stage_level=None, rheology=(0, 1.0, 1.0, 1.0, 1.0), cont0=0, cont=1, x=None, ks=None, pc=None,
                           saddle_type=0, snes_rtol=1e-8, snes_atol=1e-50, snes_max_it=50, ksp_rtol=1e-5, ksp_restart=30, ksp_max_it=10000,
                           vel=(4, 1e-5), schur=(3, 1e-5), svel=(0, 1e-5), pc_sweeps=0, line_search=True, monitor=None, max_linear_fail=1,
                           schur_jacobi=True, stats=None, dist=None):
    """Grid-sequenced stokes_solve: levels = [(op, dirichlet), ...] coarsest first, StokesOps with Dirichlet values `dirichlet` and
    their force set.  stage_level[i] (non-decreasing) is the level of continuation stage i (default: default_stage_level).  Stage i
    is solved on every level above the previous stage's level up to its own (stage 0: from the coarsest), and the state is
    prolonged (prolong_stokes) whenever the level changes; with one stage (linear rheology) that is PETSc's grid sequencing.
    x: a device tensor of the finest level's global size that receives the state (the last stage runs on the finest level).
    ks, pc: one Fgmres / StokesSaddlePc per level to use and keep, or None (made and destroyed here).  Other arguments as stokes_solve.
    Returns stokes_solve's log with a level column: (exponent, regularization, newton_its, ksp_its, |F|, level) per solve."""
    if dist is not None:
        raise ValueError("grid sequencing runs on one GPU: no slab-distributed levels")
    kind, hardness, exponent, regularization, gamma0 = rheology
    stages = continuation_schedule(exponent, regularization, cont0, cont) if kind == 1 else [(exponent, regularization)]
    nl = len(levels)
    stage_level = default_stage_level(len(stages), nl) if stage_level is None else [int(v) for v in stage_level]
    if len(stage_level) != len(stages) or any(b < a for a, b in zip(stage_level, stage_level[1:])) or stage_level[0] < 0 or stage_level[-1] != nl - 1:
        raise ValueError("stage_level %r: one non-decreasing level index per stage (%d stages), the last one %d" % (stage_level, len(stages), nl - 1))
    if x is None or x.numel() != levels[-1][0].global_size:
        raise ValueError("x: a device tensor of the finest level's global size receives the state")
    kss = list(ks) if ks is not None else [None] * nl
    pcs = list(pc) if pc is not None else [None] * nl
    own = [(kss[l] is None, pcs[l] is None) for l in range(nl)]
    gnorm = lambda t: float(t.norm())
    fails = [0]
    out = []
    cur, xl = -1, None
    try:
        for i, st in enumerate(stages):
            first = stage_level[i - 1] + 1 if i else 0
            for lev in (range(first, stage_level[i] + 1) if stage_level[i] >= first else [stage_level[i]]):
                op, dv = levels[lev]
                if lev != cur:
                    if cur < 0:
                        xl = torch.zeros(op.global_size, dtype=torch.float64, device=x.device)
                    else:
                        xl = prolong_stokes(sp, levels[cur][0].dims, xl, levels[cur][1], op.dims)
                    cur = lev
                    if lev == nl - 1:
                        x.copy_(xl); xl = x
                    if kss[lev] is None:
                        kss[lev] = sp.Fgmres(op.global_size, restart=ksp_restart, rtol=ksp_rtol, max_it=ksp_max_it)
                    if pcs[lev] is None:
                        pcs[lev] = sp.StokesSaddlePc(op, saddle_type, vel, schur, svel, pc_sweeps, schur_jacobi)
                log = _stokes_stages(op, xl, [st], kind, hardness, gamma0, kss[lev], pcs[lev], gnorm, fails, snes_rtol, snes_atol,
                                     snes_max_it, line_search, monitor, max_linear_fail)
                out.extend(row + (lev,) for row in log)
    finally:
        for l in range(nl):
            if own[l][0] and kss[l] is not None:
                kss[l].destroy()
            if own[l][1] and pcs[l] is not None:
                pcs[l].destroy()
        if stats is not None:
            stats["linear_fails"] = fails[0]
    return out


def resolution(dims, u_full):
    """How well the full-grid field u_full (all nodes of the CGL grid dims, row-major; nfields stacked fields if it holds a multiple
    of prod(dims) values) is resolved: per direction sqrt(E over the top third of the modes / total E), E the direction's energy
    spectrum of the Chebyshev coefficients (one ChebModal.forward + spectrum); a (nfields, d) host array for several fields, d values
    for one.  The number to look at before choosing the next level of a grid sequence: ~1e-16 for a resolved field, O(1) for noise.
    Nothing here is wired into the sequenced solvers."""
    from . import ChebModal
    dims = tuple(int(n) for n in dims)
    size = 1
    for n in dims:
        size *= n
    if u_full.numel() == 0 or u_full.numel() % size:
        raise ValueError("u_full: %d values are no multiple of prod(dims) = %d" % (u_full.numel(), size))
    nf = u_full.numel() // size
    m = ChebModal(dims, nf)
    try:
        a = m.forward(u_full.reshape(-1), torch.empty(m.size(), dtype=torch.float64, device=u_full.device))
        E = m.spectrum(a).cpu().view(nf, -1)
    finally:
        m.destroy()
    out = torch.zeros((nf, len(dims)), dtype=torch.float64)
    o = 0
    for k, n in enumerate(dims):
        Ek = E[:, o:o + n]
        o += n
        top = n - max(1, n // 3)
        tot = Ek.sum(dim=1)
        out[:, k] = torch.where(tot > 0, torch.sqrt(Ek[:, top:].sum(dim=1) / torch.where(tot > 0, tot, torch.ones_like(tot))), torch.zeros_like(tot))
    out = out.numpy()
    return out[0] if nf == 1 else out


def point_sources(sp, dims, pts, strengths, out=None, periodic=None):
    """Discrete point sources on the CGL grid dims: the full-grid field g with integral(g phi) = sum_p strengths[p] phi(pts[p]) for
    every polynomial phi of the grid (ChebPoints.spread with delta=True; one handle made and destroyed: for a one-off call).  pts is
    an (npts, d) device tensor, strengths npts values (one field) or (nfields, npts); returns a device tensor of shape
    (nfields,) + dims: a new one, or `out`, which must be contiguous, hold nfields prod(dims) values and is overwritten.
    periodic: ChebPoints' flags; phi is then trigonometric along a flagged direction and the integral ChebModal(periodic)'s."""
    dims = tuple(int(n) for n in dims)
    if pts.dim() != 2 or pts.shape[1] != len(dims):
        raise ValueError("pts: expected shape (npts, %d), got %r" % (len(dims), tuple(pts.shape)))
    npts = pts.shape[0]
    if strengths.dim() not in (1, 2) or strengths.shape[-1] != npts:
        raise ValueError("strengths: expected shape (%d,) or (nfields, %d), got %r" % (npts, npts, tuple(strengths.shape)))
    nf = strengths.shape[0] if strengths.dim() == 2 else 1
    if out is not None and not out.is_contiguous():
        raise ValueError("out must be contiguous")
    h = sp.ChebPoints(dims, nf, periodic=periodic)
    try:
        g = h.spread(strengths.reshape(nf, npts).contiguous(), pts.contiguous(), out=None if out is None else out.view(-1), delta=True)
        torch.cuda.current_stream().synchronize()       # (the handle's buffers are freed below)
    finally:
        h.destroy()
    return g.view((nf,) + dims)


def velocity_gradient(sp, dims, vel_full, pts, scale=None, periodic=None):
    """The velocity-gradient tensor A[p][i][j] = d u_i / d x_j at the points pts (an (npts, d) device tensor of reference
    coordinates) of the d stacked full-grid components vel_full (d prod(dims) values, component-major): one ChebPoints.eval_grad.
    scale: the d factors 2 / L_k of a box (None: the reference cube).  periodic: ChebPoints' flags.  Returns an (npts, d, d) device
    tensor."""
    dims = tuple(int(n) for n in dims)
    d = len(dims)
    size = d
    for n in dims:
        size *= n
    if vel_full.numel() != size:
        raise ValueError("vel_full: expected %d stacked components of prod(dims) values, got %d values" % (d, vel_full.numel()))
    h = sp.ChebPoints(dims, d, periodic=periodic)
    try:
        out = h.eval_grad(vel_full.reshape(-1), pts, scale=scale)
        torch.cuda.current_stream().synchronize()       # (the handle's buffers are freed below)
    finally:
        h.destroy()
    return out.permute(2, 0, 1).contiguous()


def sample_plane(sp, dims, u_full, axis, coord, m=None, deriv=None, periodic=None):
    """The plane x_axis = coord of the full-grid field u_full (all nodes of the CGL grid dims, row-major; nfields stacked fields if it
    holds a multiple of prod(dims) values): one ChebPoints.eval_grid with a single coordinate along `axis`.  The other directions
    keep their CGL nodes (m = None) or take m uniform points from -1 to +1 each.  Returns a device tensor of shape
    (nfields, points of the other directions ...), the direction `axis` dropped.  deriv: one flag (0 or 1) per direction: the
    derivative along the flagged directions with respect to the reference coordinates instead of the value (a vorticity cut is two
    such planes).  periodic: ChebPoints' flags; a flagged direction keeps its nodes fourier_nodes(n) (m = None), and `coord` along a
    periodic axis is wrapped into the period."""
    dims = tuple(int(n) for n in dims)
    axis = int(axis)
    per = (False,) * len(dims) if periodic is None else tuple(bool(p) for p in periodic)
    if len(per) != len(dims):
        raise ValueError("periodic: expected %d flags, got %d" % (len(dims), len(per)))
    if not 0 <= axis < len(dims):
        raise ValueError("axis %d out of range 0..%d" % (axis, len(dims) - 1))
    size = 1
    for n in dims:
        size *= n
    if u_full.numel() == 0 or u_full.numel() % size:
        raise ValueError("u_full: %d values are no multiple of prod(dims) = %d" % (u_full.numel(), size))
    nf = u_full.numel() // size
    dev = u_full.device
    coords = []
    for k, n in enumerate(dims):
        if k == axis:
            coords.append(torch.tensor([float(coord)], dtype=torch.float64, device=dev))
        elif m is None:
            coords.append(torch.from_numpy(sp.fourier_nodes(n) if per[k] else sp.cgl_nodes(n)).to(dev))
        else:
            coords.append(torch.linspace(-1.0, 1.0, int(m), dtype=torch.float64, device=dev))
    pts = sp.ChebPoints(dims, nf, periodic=periodic)
    try:
        out = pts.eval_grid(u_full.reshape(-1), coords, deriv=deriv)
        torch.cuda.current_stream().synchronize()       # (the handle's buffers are freed below)
    finally:
        pts.destroy()
    return out.squeeze(axis + 1)


def _stacked(dims, u_full):
    dims = tuple(int(n) for n in dims)
    size = 1
    for n in dims:
        size *= n
    if u_full.numel() == 0 or u_full.numel() % size:
        raise ValueError("u_full: %d values are no multiple of prod(dims) = %d" % (u_full.numel(), size))
    return dims, u_full.numel() // size


def profile(sp, dims, u_full, axis):
    """The mean profile along `axis` of the full-grid field u_full (all nodes of the CGL grid dims, row-major; nfields stacked fields
    if it holds a multiple of prod(dims) values): the mean over every other direction (one ChebReduce.apply with "mean" weights),
    a device tensor of shape (nfields, dims[axis])."""
    dims, nf = _stacked(dims, u_full)
    axis = int(axis)
    if not 0 <= axis < len(dims):
        raise ValueError("axis %d out of range 0..%d" % (axis, len(dims) - 1))
    if len(dims) == 1:
        return u_full.reshape(nf, dims[0]).clone()
    over = [k for k in range(len(dims)) if k != axis]
    red = sp.ChebReduce(dims, nf, over=over, weights={k: "mean" for k in over})
    try:
        out = red.apply(u_full.reshape(-1))
        torch.cuda.current_stream().synchronize()       # (the handle's buffers are freed below)
    finally:
        red.destroy()
    return out


def face_flux(sp, dims, u_full, axis, side, integrate=True):
    """The outward normal derivative du/dnu of the full-grid field u_full (layout as profile) on the face x_axis = +1 (side = 0,
    grid index 0) or x_axis = -1 (side = 1, the last index): one pass over the field with a row of D as the weights of `axis`,
    + at side 0 and - at side 1 (the convention of HelmholtzSolver's boundary conditions).  integrate = True: its integral over
    the face, a device tensor of nfields values; False: the face field, shape (nfields, the other directions ...)."""
    dims, nf = _stacked(dims, u_full)
    axis, side = int(axis), int(side)
    if not 0 <= axis < len(dims):
        raise ValueError("axis %d out of range 0..%d" % (axis, len(dims) - 1))
    if side not in (0, 1):
        raise ValueError("side %d: 0 (x = +1) or 1 (x = -1)" % side)
    w = sp.reduce_weights(dims[axis], "dnode", 0 if side == 0 else dims[axis] - 1)
    over = list(range(len(dims))) if integrate else [axis]
    red = sp.ChebReduce(dims, nf, over=over, weights={axis: w if side == 0 else -w})
    try:
        out = red.apply(u_full.reshape(-1))
        torch.cuda.current_stream().synchronize()       # (the handle's buffers are freed below)
    finally:
        red.destroy()
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# From a solver state to the full-grid toolbox (ChebLayout) and the vector calculus of the result (ChebGrad), all on the device
# ---------------------------------------------------------------------------------------------------------------------------------

_layout_cache = {}


def _layout(sp, dims, device):
    """The ChebLayout of a grid, built once per (dims, device)."""
    key = (tuple(int(n) for n in dims), str(device))
    if key not in _layout_cache:
        _layout_cache[key] = sp.ChebLayout(key[0])
    return _layout_cache[key]


def stokes_fields(sp, op, x, dirichlet):
    """The Stokes state x ([v_0 .. v_{d-1}, p] per interior node, a device tensor of op.global_size values) as full-grid fields: a
    (d + 1, *dims) device tensor whose first d fields are the velocity with its Dirichlet values (`dirichlet`: the compact array
    of stokes_op_set_dirichlet, d values per boundary node; a host array is uploaded) and whose last field is the pressure with
    ZERO on the boundary -- a placeholder, not an extrapolation.  Two ChebLayout.unpack launches, nothing through the host."""
    d = op.d
    lay = _layout(sp, op.dims, x.device)
    out = torch.empty((d + 1,) + tuple(op.dims), dtype=torch.float64, device=x.device)
    xb = _dev_values(dirichlet, x).reshape(-1).contiguous()
    xv = x.reshape(-1)
    lay.unpack(d, xv, d + 1, 0, xb, d, 0, out=out[:d])
    lay.unpack(1, xv, d + 1, d, None, 1, 0, out=out[d:])
    return out


def elliptic_field(sp, op, x, dirichlet):
    """The elliptic state x (interior nodes, a device tensor of op.global_size values) with its compact Dirichlet values
    (ell_op_set_dirichlet order; a host array is uploaded) as one full-grid field: a (*dims) device tensor."""
    lay = _layout(sp, op.dims, x.device)
    out = torch.empty((1,) + tuple(op.dims), dtype=torch.float64, device=x.device)
    lay.unpack(1, x.reshape(-1), 1, 0, _dev_values(dirichlet, x).reshape(-1).contiguous(), 1, 0, out=out)
    return out[0]


def strain_invariant(sp, dims, vel_full, scale=None):
    """gamma = 1/2 S:S (stokes.C:711-717) of the full-grid velocity vel_full (d fields, all nodes of the CGL grid dims), the number
    the power-law viscosity is a function of: a (*dims) device tensor.  One ChebGrad.tensor and one invariants launch; scale[k]
    multiplies the derivative along direction k."""
    dims = tuple(int(n) for n in dims)
    g = sp.ChebGrad(dims, scale)
    try:
        if vel_full.numel() != g.N * len(dims):
            raise ValueError("vel_full: expected %d fields of %d values" % (len(dims), g.N))
        out = g.invariants(vel_full.reshape(-1), ("gamma",))
        torch.cuda.current_stream().synchronize()       # (the handle's matrices are freed below)
    finally:
        g.destroy()
    return out[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# Field statistics (ChebStats)
# ---------------------------------------------------------------------------------------------------------------------------------

def pdf(sp, dims, u_full, bins, range=None):
    """The volume-weighted probability density of the full-grid field u_full (layout as profile): (centres, density), device
    tensors of shape (nfields, bins), the density normalised to integrate to 1 over the mass that fell inside the range (all
    zeros if none did).  range: (lo, hi) for every field, or None for ChebStats.auto_range of each field's
    summary, taken on the device.  A node counts with its Clenshaw-Curtis volume, not once: the CGL grid packs its
    nodes against the walls, and an unweighted histogram of the node values is the PDF of the grid."""
    dims, nf = _stacked(dims, u_full)
    bins = int(bins)
    st = sp.ChebStats(dims, nf, max_bins=bins)
    try:
        u = u_full.reshape(-1)
        if range is None:
            lohi = st.auto_range(st.summary(u))
        else:
            lo, hi = (float(x) for x in range)
            lohi = torch.tensor([[lo, hi]] * nf, dtype=torch.float64, device=u.device)
        h = st.histogram(u, bins, range=lohi)
        torch.cuda.current_stream().synchronize()       # (the handle's buffers are freed below)
    finally:
        st.destroy()
    mass = h[:, 0, 1:bins + 1]
    width = ((lohi[:, 1] - lohi[:, 0]) / bins).unsqueeze(1)
    k = torch.arange(bins, dtype=torch.float64, device=u.device).unsqueeze(0)
    centres = lohi[:, :1] + (k + 0.5) * width
    total = mass.sum(dim=1, keepdim=True)
    density = torch.where(total > 0, mass / (total * width), torch.zeros_like(mass))
    return centres, density


def cfl_dt(sp, dims, vel_full, cfl=0.5, scale=None):
    """The advective time-step limit of the full-grid velocity vel_full (d fields, all nodes of the CGL grid dims):
    dt = cfl / max_i sum_k |vel_k(i)| s_k / h_k(i_k), h_k the local node spacing, s_k = scale[k] = 2 / L_k (ChebStats.cfl).
    Returns (dt, index of the limiting node) as Python numbers (one sync); dt is NaN if the velocity holds a NaN -- no step
    must be chosen from a field that has blown up -- and inf for a velocity that is zero everywhere."""
    dims = tuple(int(n) for n in dims)
    st = sp.ChebStats(dims, 1, max_bins=1)              # (one bin: the histogram's buffers of this handle are a few KB)
    try:
        out = st.cfl(vel_full.reshape(-1), scale).cpu()
    finally:
        st.destroy()
    m, idx = float(out[0]), int(out[1])
    if m != m:
        return float("nan"), idx
    return (float(cfl) / m if m > 0 else float("inf")), idx
