"""The Stokes node laws on the CPU (csrc/stokes_node.h: the rheology and the node laws of StokesMatMultVV and StokesFunction that every
node kernel of stokes.hip calls): tests/host/stokes_node_check.cpp holds them to the same formulas in long double, with the bars of
callbacks_ref's docstring at a node -- every stress entry (d^2 + 4) 2^-53 of |eta| |s_jk| + |eta'| |S0_jk| sum |S0| |s| (the residual with
S0 = s), strain 1, trace d, eta and eta' relative by the dq formula with the gradient exact -- and checks the
bit-for-bit properties the routes rely on (DETA off = DETA on with eta' = 0; D = 3 with an empty third row and column = D = 2; the pair
forms = the scalar ones).  D = 2 and 3, 400 nodes each, gradients over 10^+-30 for the linear laws and of order 1 for the power law,
the rheologies LINEAR and POWER of test_gpu_callbacks.py.
The pow allowance is the host library's own, measured by the program on its q values (worst error against powl in ulps, doubled and
rounded up: the rule behind callbacks_ref.POW_ULPS, which is the device's figure, and no more than it: a host pow worse than the device's
would widen the bars unseen); profiles/stokes_node/host_pow_ulps.txt records it.
Compiles the program with hipcc (host code only); no GPU."""
import math
import os
import shutil
import subprocess
import pytest

import callbacks_ref as cb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CASES = ["vv 2", "vv 3", "fn_linear 2", "fn_linear 3", "fn_power 2", "fn_power 3", "embedding 3", "pairs 3"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_node_laws_against_long_double(tmp_path):
    csrc = os.path.join(ROOT, "spectral-petsc_amd", "csrc")
    exe = str(tmp_path / "stokes_node_check")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", csrc, os.path.join(ROOT, "tests", "host", "stokes_node_check.cpp"),
                    "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    lines = [l.split() for l in r.stdout.split("\n") if l.strip()]
    cases = [l for l in lines if l[0] == "case"]
    assert ["%s %s" % (l[1], l[3]) for l in cases] == CASES
    for l in cases:
        assert l[-1] == "pass" and int(l[5]) >= 200, " ".join(l)
    pow_line = [l for l in lines if l[0] == "pow_ulps"]
    assert len(pow_line) == 1
    worst, allowance = float(pow_line[0][1]), int(pow_line[0][3])
    assert worst > 0.0 and allowance == math.ceil(2.0 * worst), pow_line      # the allowance the program's bars used is the rule's
    assert allowance <= cb.POW_ULPS, pow_line
    assert lines[-1] == ["ok"] and r.returncode == 0
