#!/usr/bin/env python3
"""Per-kernel comparison of two builds' device assembly, as a markdown table.

usage: isa_compare.py DIR_PARENT DIR_CHANGE [old_name=new_name ...]
    DIR_PARENT, DIR_CHANGE: one FILE.s per csrc/FILE.hip, compiled with the Makefile's flags plus `--cuda-device-only -S`.
    old_name=new_name: a kernel (or file) renamed between the builds, by its name without arguments (`fps_sort_kernel=cs_sort_points_kernel`, `'k<1>=k'`).

Two kernels are "identical" when their instruction streams are equal after dropping comments, directives (.loc, .file,
.p2align, ...) and the numbering of local labels.  The resource columns come from the .amdgpu_metadata of each file,
the instruction counts from the same opcode filter as tools/isa_linecount.py.  Device functions that were not inlined
are compared like kernels (their resources are part of their callers')."""
import glob, os, re, subprocess, sys, collections

OPCODE = re.compile(r'^(v_|s_|ds_|buffer_|global_|flat_|scratch_)')


def demangle(names):
    names = list(names)
    tool = '/opt/rocm/llvm/bin/llvm-cxxfilt'
    out = subprocess.run([tool if os.path.exists(tool) else 'c++filt'] + names, capture_output=True, text=True, check=True)
    return dict(zip(names, out.stdout.strip().split('\n')))


def functions(path):
    """mangled name -> (normalised instruction stream, metadata dict or None)"""
    body, meta = {}, {}
    cur = None
    labels = {}
    in_meta, kern = False, None
    for line in open(path):
        s = line.split(';', 1)[0].rstrip() if not in_meta else line.rstrip('\n')
        if s.strip() == '.amdgpu_metadata':
            in_meta = True
            continue
        if s.strip() == '.end_amdgpu_metadata':
            in_meta = False
            continue
        if in_meta:
            if re.match(r'^  - \.', s):
                kern = {}
            m = re.match(r'^  (?:- | {2})\.(\w+):\s+(\S+)$', s)
            if m and kern is not None:
                kern[m.group(1)] = m.group(2)
                if m.group(1) == 'name':
                    meta[m.group(2)] = kern
            continue
        s = s.strip()
        m = re.match(r'^([_A-Za-z$][\w$.]*):$', s)
        if m and not s.startswith('.L'):
            cur = m.group(1)
            body[cur] = []
            labels = {}
            continue
        if cur is None or not s:
            continue
        if s.startswith('.Lfunc_end'):
            cur = None
            continue
        if s.startswith('.') and not s.startswith('.LBB'):
            continue
        s = re.sub(r'\.LBB\d+_\d+', lambda k: labels.setdefault(k.group(0), 'L%d' % len(labels)), s)
        body[cur].append(re.sub(r'\s+', ' ', s))
    return {k: (v, meta.get(k)) for k, v in body.items() if any(OPCODE.match(l) for l in v)}


def base(demangled):
    head = demangled.split('(')[0]
    return re.sub(r'^void ', '', head)


def load(d, renames):
    out = {}
    for path in sorted(glob.glob(os.path.join(d, '*.s'))):
        fns = functions(path)
        names = demangle(fns)
        for k, (stream, meta) in fns.items():
            name = base(names[k]).replace('mvp::', '')
            stem = re.sub(r'<.*', '', name)
            name = renames.get(name) or renames.get(stem, stem) + name[len(stem):]
            # the mangled symbol occurs in the stream (s_getpc / relocations of calls): name it alike on both sides
            stream = [l.replace(k, '<self>') for l in stream]
            out[name] = (os.path.basename(path)[:-2], stream, meta)
    return out


def main(argv):
    renames = dict(a.split('=', 1) for a in argv[2:])
    a, b = load(argv[0], renames), load(argv[1], {})
    print('| kernel | file | identical | instructions | VGPRs | SGPRs | LDS bytes | scratch bytes | spills (v+s) |')
    print('|---|---|---|---|---|---|---|---|---|')
    summary = collections.Counter()
    for name in sorted(set(a) | set(b), key=lambda n: ((a.get(n) or b.get(n))[0], n)):
        fa, fb = a.get(name), b.get(name)
        if fa is None or fb is None:
            print('| `%s` | %s | only in %s | | | | | | |' % (name, (fa or fb)[0], 'parent' if fa else 'change'))
            summary['unmatched'] += 1
            continue
        # calls name their (mangled) callee: compare those by position only
        strip = lambda st: [re.sub(r'_ZN?3mvp\w+', '<fn>', l) for l in st]
        same = strip(fa[1]) == strip(fb[1])
        summary['identical' if same else 'different'] += 1

        def col(key, f=lambda m, k: m[k]):
            va = f(fa[2], key) if fa[2] else '-'
            vb = f(fb[2], key) if fb[2] else '-'
            return '%s \\| %s' % (va, vb)
        ni = '%d \\| %d' % (sum(1 for l in fa[1] if OPCODE.match(l)), sum(1 for l in fb[1] if OPCODE.match(l)))
        spills = col(None, lambda m, k: int(m['vgpr_spill_count']) + int(m['sgpr_spill_count']))
        files = fa[0] if fa[0] == fb[0] else '%s -> %s' % (fa[0], fb[0])
        print('| `%s` | %s | %s | %s | %s | %s | %s | %s | %s |' % (
            name, files, 'yes' if same else 'NO', ni, col('vgpr_count'), col('sgpr_count'),
            col('group_segment_fixed_size'), col('private_segment_fixed_size'), spills))
    print()
    print('%d identical, %d different, %d without a counterpart' % (summary['identical'], summary['different'], summary['unmatched']))


if __name__ == '__main__':
    main(sys.argv[1:])
