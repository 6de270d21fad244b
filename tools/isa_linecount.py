#!/usr/bin/env python3
"""Static instruction count per source line of one kernel in a hipcc -save-temps -gline-tables-only .s file.

usage: isa_linecount.py file.s kernel_substring [lo hi [main_file]]
           lo..hi: only lines of the main file in that range; inlined header lines are attributed to the last
           main-file line seen
       isa_linecount.py --by-file file.s kernel_substring [--split FILE:LINE] [--instance K] [--lines FILE]
           one row per source file (every instruction under the file its own .loc names), with the columns of
           profiles/emd_*_instruction_budget.md: VALU / SALU / LDS / VMEM / s_waitcnt / s_nop / scratch, the SGPR-spill
           lane moves (v_writelane / v_readlane) and the workgroup barriers.
           --split FILE:LINE   cut the kernel into instances of an inlined function: a new instance starts where a .loc
                               of that line follows at least 2000 instructions without one (e.g. emd_lean.hip:105,
                               the first statement of emd_lean_body that survives); --instance K counts only the K-th
           --lines FILE        also one row per line of that file
"""
import re, sys, collections

KINDS = ('valu', 'salu', 'lds', 'vmem', 'waitcnt', 'nop', 'scratch', 'lane', 'barrier')


def kind_of(op):
    if op.startswith('v_writelane') or op.startswith('v_readlane'):
        return 'lane'
    if op.startswith('s_waitcnt'):
        return 'waitcnt'
    if op.startswith('s_nop'):
        return 'nop'
    if op.startswith('s_barrier'):
        return 'barrier'
    if op.startswith('v_'):
        return 'valu'
    if op.startswith('s_'):
        return 'salu'
    if op.startswith('ds_'):
        return 'lds'
    if op.startswith('scratch_'):
        return 'scratch'
    return 'vmem'


def instructions(path, kern):
    """(file name, line, opcode) of every instruction of the kernels whose label contains `kern`."""
    files = {}
    inside = False
    cur = ('', 0)
    for line in open(path):
        s = line.strip()
        m = re.match(r'\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', s)
        if m:
            files[int(m.group(1))] = (m.group(3) or m.group(2)).rsplit('/', 1)[-1]
            continue
        if re.match(r'^[_A-Za-z0-9$.]+:', s) and not s.startswith('.L'):
            inside = kern in s
            continue
        if not inside:
            continue
        m = re.match(r'\.loc\s+(\d+)\s+(\d+)', s)
        if m:
            cur = (files.get(int(m.group(1)), '?'), int(m.group(2)))
            continue
        if s.startswith('.') or s.startswith(';') or not s:
            continue
        op = s.split()[0]
        if re.match(r'^(v_|s_|ds_|buffer_|global_|flat_|scratch_)', op):
            yield cur[0], cur[1], op


def row(name, k):
    return "%-34s %6d  " % (name, sum(k.values())) + " ".join("%s %5d" % (n, k[n]) for n in KINDS)


def by_file(argv):
    path, kern = argv[0], argv[1]
    split = lines_of = None
    instance = -1
    i = 2
    while i < len(argv):
        if argv[i] == '--split':
            f, l = argv[i + 1].split(':')
            split = (f, int(l))
        elif argv[i] == '--instance':
            instance = int(argv[i + 1])
        elif argv[i] == '--lines':
            lines_of = argv[i + 1]
        i += 2
    per_file = collections.defaultdict(collections.Counter)
    per_line = collections.defaultdict(collections.Counter)
    inst, since = -1, 10 ** 9
    sizes = collections.Counter()
    for f, l, op in instructions(path, kern):
        if split is not None:
            if (f, l) == split:
                if since >= 2000:
                    inst += 1
                since = 0
            else:
                since += 1
            sizes[inst] += 1
            if instance >= 0 and inst != instance:
                continue
        k = kind_of(op)
        per_file[f][k] += 1
        if f == lines_of:
            per_line[l][k] += 1
    if split is not None:
        print('instances (instructions each):', dict(sizes))
    tot = collections.Counter()
    for f in sorted(per_file, key=lambda f: -sum(per_file[f].values())):
        print(row(f, per_file[f]))
        tot.update(per_file[f])
    print(row('total', tot))
    for l in sorted(per_line):
        print(row('%s:%d' % (lines_of, l), per_line[l]))


def by_line(argv):
    path, kern = argv[0], argv[1]
    lo = int(argv[2]) if len(argv) > 2 else 0
    hi = int(argv[3]) if len(argv) > 3 else 10**9
    main = argv[4] if len(argv) > 4 else 'emd.hip'
    anchor = 0
    cnt = collections.Counter()
    kinds = collections.defaultdict(collections.Counter)
    for f, l, op in instructions(path, kern):
        if f.endswith('emd.hip') or f.endswith(main):
            anchor = l
        if lo <= anchor <= hi:
            cnt[anchor] += 1
            k = 'valu' if op.startswith('v_') else 'salu' if op.startswith('s_') else 'lds' if op.startswith('ds_') else 'scratch' if op.startswith('scratch_') else 'vmem'
            kinds[anchor][k] += 1
    tot = collections.Counter()
    for ln in sorted(cnt):
        k = kinds[ln]
        print(f"{ln:5d} {cnt[ln]:5d}  valu {k['valu']:4d} salu {k['salu']:4d} lds {k['lds']:3d} vmem {k['vmem']:3d} scratch {k['scratch']:3d}")
        tot.update(k)
    print('total', sum(cnt.values()), dict(tot))


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--by-file':
        by_file(sys.argv[2:])
    else:
        by_line(sys.argv[1:])
