"""The machine code of the long-line sweep kernels (csrc/sweep_vec.hip), read from a hipcc -S listing; no GPU.

Two things in vec4_body hold only as long as hipcc keeps emitting what it emits today, and nothing on the GPU would show the day it
stops:
  * the stores of the strided kernel run under a lane mask that is written to EXEC by hand (the columns a row's last tile lacks).
    The compiler does not know that the region runs with part of the lanes: a register copy, a reload or any other vector
    instruction placed inside it would leave stale values in the other lanes -- wrong results, and only in tiles where a row
    ends early.  Every region must hold its two buffer stores and nothing else but s_nop / s_waitcnt;
  * the buffer descriptors are re-based on the scalar unit (csrc/tile.h rsrc_at), which rests on an empty asm that hides one
    operand from the optimiser.  If that stops working the descriptor words move into vector registers and every access becomes
    a v_readfirstlane loop: correct, and slow.  No loop of these kernels may contain a v_readfirstlane, a lane spill
    (v_readlane / v_writelane) or a wait for everything (s_waitcnt vmcnt(0)), and no kernel may use private memory.
One compilation of the file (about a minute and a half) serves all the checks."""
import os
import re
import shutil
import subprocess

import pytest

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spectral-petsc_amd", "csrc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("listing") / "sweep_vec.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-I", CSRC,
                    os.path.join(CSRC, "sweep_vec.hip"), "-o", out], check=True, timeout=900, capture_output=True)
    with open(out) as f:
        return f.read().split("\n")


def code(line):
    return line.split(";")[0].strip()


def kernels(lines):
    """(mangled name, first line, last line) of every kernel that contains vec4_body."""
    out = []
    for i, l in enumerate(lines):
        m = re.match(r"(_ZN7chebhip\w+):", l)
        if m and ("vec4" in m.group(1) or re.search(r"multi\w*kernelILi(16|32)E", m.group(1))):
            end = next(j for j in range(i + 1, len(lines)) if lines[j].startswith(".Lfunc_end"))
            out.append((m.group(1), i, end))
    return out


def loops(lines, a, b):
    """The long loops (tile loops) of the function in lines[a:b]: (first, last) line of each backward branch over more than 300 lines."""
    labels = {}
    for i in range(a, b):
        m = re.match(r"(\.LBB\d+_\d+):", lines[i])
        if m:
            labels[m.group(1)] = i
    out = []
    for i in range(a, b):
        m = re.search(r"s_c?branch\w* (\.LBB\d+_\d+)", lines[i])
        if m and m.group(1) in labels and labels[m.group(1)] < i and i - labels[m.group(1)] > 300:
            out.append((labels[m.group(1)], i))
    return out


def test_regions_under_a_hand_set_exec_hold_two_stores_only(listing):
    regions, i, n = 0, 0, len(listing)
    while i < n:
        if re.match(r"s_mov_b64 exec, s\[", code(listing[i])):
            regions += 1
            body, j = [], i + 1
            while code(listing[j]) != "s_mov_b64 exec, -1":
                c = code(listing[j])
                if c and not c.startswith("."):
                    body.append(c)
                j += 1
                assert j - i < 40, "line %d: EXEC is set from a scalar and not restored within 40 lines" % (i + 1)
            stores = [c for c in body if c.startswith("buffer_store_dwordx4")]
            other = [c for c in body if not c.startswith(("buffer_store_dwordx4", "s_nop", "s_waitcnt"))]
            assert len(stores) == 2 and not other, "line %d: a region under a partial EXEC holds %s" % (i + 1, body)
            i = j
        i += 1
    # COLFAST kernels: 16 without a gather loader (KS = 16 / 32 x 8 modes) + the COLFAST bodies of the multi-job kernels; each has
    # two wave-group copies x (peeled first tile + loop) x 2 sub-tiles x 2 row pairs.  The count guards the pattern above against
    # a listing in which the regions are simply written another way
    assert regions >= 16 * 16, regions


def test_tile_loops_stay_scalar_addressed_and_exactly_counted(listing):
    ks = kernels(listing)
    assert len(ks) >= 40, len(ks)
    nloops = 0
    for name, a, b in ks:
        for la, lb in loops(listing, a, b):
            body = [code(l) for l in listing[la:lb]]
            mfma = sum(1 for c in body if c.startswith("v_mfma_f64"))
            if mfma < 64:
                continue
            nloops += 1
            for pat, what in ((r"v_readfirstlane", "a descriptor or an offset came from vector registers (waterfall)"),
                              (r"v_readlane|v_writelane", "a scalar register is spilled inside the loop"),
                              (r"s_waitcnt vmcnt\(0\)", "the loop waits for everything in flight")):
                hits = [c for c in body if re.match(pat, c)]
                assert not hits, "%s, loop at line %d: %s (%s)" % (name, la + 1, what, hits[0])
    assert nloops >= 2 * len(ks), nloops


def test_no_kernel_uses_private_memory(listing):
    text = "\n".join(listing)
    sizes = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(sizes) >= 40
    assert [s for s in sizes if s[1] != "0"] == []
