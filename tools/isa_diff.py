#!/usr/bin/env python3
"""Per-kernel comparison of two device listings of the same source file:
    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S x.hip -o a.s     (before)
    ...                                                                   -o b.s     (after)
    tools/isa_diff.py a.s b.s [more pairs ...]
One line per kernel symbol: "identical", or "differs" with VGPR/AGPR/SGPR/LDS/scratch of both sides and the number of
changed instruction lines.  Comment lines and the __hip_cuid_* symbol (a content hash) are dropped before comparing; block labels lose
the number of their function (.LBB12_3 -> .LBB_3: it shifts when kernels are instantiated in another order) and a kernel's own symbol
is written <self>.  A kernel whose parameter list changed has another symbol: the two are paired when its name and template arguments
occur once on either side, and the line says so.
Exit status 1 when the symbol sets or any resource numbers differ."""
import difflib
import re
import subprocess
import sys


def kernels(path):
    """{symbol: (instruction lines, {resource: value})}"""
    out, name, body = {}, None, []
    res_of = {}
    last = None
    for raw in open(path):
        line = raw.split(';', 1)[0].rstrip() if not raw.lstrip().startswith(';') else ''
        m = re.match(r'\s*\.type\s+(\S+),@function', raw)
        if m:
            name, body = m.group(1), []
            continue
        if name and re.match(r'\.Lfunc_end\d+:', raw):
            out[name] = body
            last, name = name, None
            continue
        if name:
            if line.strip() and '__hip_cuid_' not in line:
                body.append(re.sub(r'\.LBB\d+_', '.LBB_', line.strip()).replace(name, '<self>'))
            continue
        m = re.match(r';\s*(NumVgprs|NumAgprs|(?:Total)?NumSgprs|ScratchSize|LDSByteSize):\s*(\d+)', raw)
        if m and last:
            res_of.setdefault(last, {})[m.group(1)] = int(m.group(2))     # (NumSgprs and TotalNumSgprs: kept apart, both compared)
    return {k: (v, res_of.get(k, {})) for k, v in out.items()}


def demangle(names):
    for tool in ('llvm-cxxfilt', 'c++filt'):
        try:
            r = subprocess.run([tool], input='\n'.join(names), capture_output=True, text=True, check=True)
            # (the parentheses of an unnamed namespace would end the name where the parameter list is cut off)
            return dict(zip(names, r.stdout.replace('(anonymous namespace)::', '').split('\n')))
        except Exception:
            pass
    return {n: n for n in names}


def fmt(r):
    r = dict(r, Sgprs=r.get('TotalNumSgprs', r.get('NumSgprs', -1)))           # printed: the total where the listing has one
    return 'v%d a%d s%d lds%d scratch%d' % tuple(r.get(k, -1) for k in ('NumVgprs', 'NumAgprs', 'Sgprs', 'LDSByteSize', 'ScratchSize'))


def main(argv):
    bad = False
    for a, b in zip(argv[0::2], argv[1::2]):
        ka, kb = kernels(a), kernels(b)
        print('== %s -> %s: %d / %d kernels' % (a, b, len(ka), len(kb)))
        # kernels whose parameter list changed: pair them by name and template arguments where that is unambiguous
        only = sorted(set(ka) ^ set(kb))
        bare = {n: re.sub(r'\(.*\)$', '', d) for n, d in demangle(only).items()}
        renamed = {}
        for n in [n for n in only if n in ka]:
            twins = [m for m in only if m in kb and bare[m] == bare[n]]
            if len(twins) == 1 and sum(1 for m in only if m in ka and bare[m] == bare[n]) == 1:
                renamed[twins[0]] = n
        for m, n in renamed.items():
            kb[n] = kb.pop(m)
        if set(ka) != set(kb):
            bad = True
            for n in sorted(set(ka) ^ set(kb)):
                print('  only in %s: %s' % ('first' if n in ka else 'second', n))
        nice = demangle(sorted(set(ka) & set(kb)))
        same = 0
        for n in sorted(set(ka) & set(kb)):
            (ia, ra), (ib, rb) = ka[n], kb[n]
            short = re.sub(r'^void chebhip::|\(.*\)$', '', nice[n])
            if ia == ib and ra == rb:
                same += 1
                print('  identical  %s%s' % (short, ' (parameter list changed)' if n in renamed.values() else ''))
                continue
            changed = sum(1 for l in difflib.unified_diff(ia, ib, lineterm='', n=0) if l[:1] in '+-' and l[:3] not in ('+++', '---'))
            if ra != rb:
                bad = True
            note = ' (parameter list changed)' if n in renamed.values() else ''
            print('  differs    %s%s: %s | %s%s; %d of %d instruction lines changed' % (short, note, fmt(ra), fmt(rb), '' if ra == rb else '  RESOURCES DIFFER', changed, len(ia)))
        print('  %d of %d identical' % (same, len(set(ka) & set(kb))))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
