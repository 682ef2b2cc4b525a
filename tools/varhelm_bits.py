#!/usr/bin/env python3
"""One SHA-256 line per case of the SCALAR mode of VarHelmholtz (set_coefficients): `mult`, `residual`, `precond` and `solve`
(with its iteration count) on three shapes -- the fused route with three fields, a periodic channel, and the two-sweep route of a
258-point line.  Compares nothing: run it on two builds (a checkout of each, this file copied into the older one's tools/) and diff
(profiles/varhelm/tensor_bits_parent.txt, tensor_bits_new.txt).  It calls nothing the tensor mode added."""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import __graft_entry__ as ge
sp = ge.load()

CASES = [((34, 36, 40), ["dirichlet", "neumann", ("dirichlet", "neumann")], (0.5, 1.0, 2.0), 3),
         ((8, 9, 6), ["periodic", (1.0, 2.0), "periodic"], None, 2),
         ((6, 5, 258), [(1.0, 2.0), ("neumann", "dirichlet"), "dirichlet"], None, 1)]


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def main():
    for dims, bc, scale, nf in CASES:
        per = sp.bc_split(bc, 3)[0]
        xs = [(-1.0 + 2.0 * np.arange(n) / n) if p else np.cos(np.pi * np.arange(n) / (n - 1)) for n, p in zip(dims, per)]
        X = np.meshgrid(*xs, indexing="ij")
        kap = 1.0 + 0.9 * np.sin(2.0 * X[0]) * np.sin(2.0 * X[1] + 0.3) * np.sin(2.0 * X[2] + 0.6)
        c = 2.0 + np.cos(X[0])
        op = sp.VarHelmholtz(dims, nf, bc=bc, scale=scale)
        op.set_coefficients(torch.from_numpy(kap).cuda().reshape(-1), torch.from_numpy(c).cuda().reshape(-1))
        rng = np.random.default_rng(20261021)
        x, f = (torch.from_numpy(rng.standard_normal(op.size)).cuda() for _ in range(2))
        g = torch.from_numpy(rng.standard_normal(op.boundary_size)).cuda()
        y = torch.empty_like(x)
        tag = "%s nf=%d" % ("x".join(map(str, dims)), nf)
        print("mult     %s %s" % (tag, sha(op.mult(x, y))))
        print("residual %s %s" % (tag, sha(op.residual(x, f, g, y))))
        print("precond  %s %s" % (tag, sha(op.precond(x, y))))
        u = torch.empty(op.full_size, dtype=torch.float64, device="cuda")
        xs_ = op.solve(f, g, u_full=u, rtol=1e-10, restart=30)
        print("solve    %s %s %s its=%d sigma=%r" % (tag, sha(xs_), sha(u), op.iterations, op.sigma))
        op.destroy()


if __name__ == "__main__":
    main()
