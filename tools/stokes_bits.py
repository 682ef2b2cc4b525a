#!/usr/bin/env python3
"""Output bits of the Stokes callbacks, for comparing two builds of the library (the node laws of csrc/stokes_node.h, the gather and
scatter kernels): for each shape -- (13, 11, 9) all odd, (14, 12, 10) even and small, (120, 121, 68) and 128^3 on
the fused z route -- each state of tests/test_gpu_callbacks.py (default, general, eta, full) and both rheologies (LINEAR, POWER), the
outputs of stokes_op_mult, _mult_vv and _mult_vv_cm on the state as set, of _function with Dirichlet values and a force, the state
arrays it leaves (get_state: eta, eta', strain[j]), and of _mult on that state.  One line per case with one SHA-256 over the output
bytes; --all prints a line per output as well, which is what to look at when two case lines differ.  Inputs are the seeded families
of tests/callbacks_ref.py.  The script compares nothing: run it on two builds, each in a fresh process, and diff the outputs
    python tools/stokes_bits.py > new.txt
    CHEBHIP_LIB_PATH=/elsewhere/libchebhip.so python tools/stokes_bits.py > parent.txt
(profiles/stokes_node/bits_parent.txt and bits_new.txt are such a pair, taken with --all).
usage: stokes_bits.py [--all]"""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import __graft_entry__ as ge
import callbacks_ref as cb
sp = ge.load()                              # (the package reads CHEBHIP_LIB_PATH when it is imported)
ALL = "--all" in sys.argv[1:]
SHAPES = [(13, 11, 9), (14, 12, 10), (120, 121, 68), (128, 128, 128)]
STATES = ("default", "general", "eta", "full")
RHEOLOGIES = {"linear": (0, 1.0, 1.0, 1.0, 1.0), "power": (1, 1.0, 3.0, 1e-2, 1.0)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def main():
    for dims in SHAPES:
        N, I, g, ndv = cb.sizes(dims)
        d = len(dims)
        x, xv = dev(cb.noise(dims, 11)), dev(np.random.default_rng(12).standard_normal(d * I))
        dirichlet, force = np.random.default_rng(13).standard_normal(ndv), np.random.default_rng(14).standard_normal(g)
        for state in STATES:
            for rname, rheology in RHEOLOGIES.items():
                sp.set_option("general_viscous", 1 if state == "general" else 0)
                op = sp.StokesOp(dims)
                sp.set_option("general_viscous", 0)
                eta, deta, S0 = cb.stokes_state(dims, "default" if state == "general" else state)
                if eta is not None:
                    op.set_state(0, eta)
                if deta is not None:
                    op.set_state(1, deta)
                    for j in range(d):
                        op.set_state(2 + j, S0[j])
                op.set_rheology(*rheology)
                op.set_dirichlet(dirichlet)
                op.set_force(force)
                tag = "%s %s %s" % ("x".join(map(str, dims)), state, rname)
                case = hashlib.sha256()

                def emit(what, a):
                    line = "%s %s %s" % (tag, what, hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())
                    case.update(line.encode())
                    if ALL:
                        print(line, flush=True)

                def call(fn, v):
                    y = torch.full_like(v, float("nan"))
                    fn(v, y)
                    torch.cuda.synchronize()
                    return y.cpu().numpy()
                emit("mult", call(op.mult, x))
                emit("mult_vv", call(op.mult_vv, xv))
                emit("mult_vv_cm", call(op.mult_vv_cm, xv))
                emit("function", call(op.function, x))
                for w in range(2 + d):
                    emit("state%d" % w, op.get_state(w))
                emit("mult_after_function", call(op.mult, x))
                op.destroy()
                print("%s %s" % (tag, case.hexdigest()), flush=True)


if __name__ == "__main__":
    main()
