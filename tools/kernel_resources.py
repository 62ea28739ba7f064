"""Resource figures and instruction counts per kernel of device assembly, for pinning a refactor of kernels that sit at the register limit:

    hipcc <dir_amd/build.py FLAGS> --cuda-device-only -S dir_amd/csrc/tail.hip -o tail.s
    python tools/kernel_resources.py tail.s [more.s ...]                 # the table
    python tools/kernel_resources.py --diff parent/tail.s child/tail.s    # what differs, kernel by kernel

The table holds what the compiler reports (VGPR, AGPR, scratch bytes, spilled VGPRs, LDS bytes, occupancy) and the counts of the
instructions that decide speed and bits: matrix, memory, LDS, waits, barriers, lane swaps, floating point and conversions.  --diff lists
every figure and every mnemonic whose count differs (integer address arithmetic included), or 'equal'."""
import collections
import re
import subprocess
import sys

PINNED = ('v_mfma', 'global_', 'buffer_', 'ds_', 'scratch_', 's_waitcnt', 's_barrier', 'v_permlane', 'v_fma', 'v_add_f32', 'v_cvt', 'v_pk_', 'v_max')
FIGURES = (('NumVgprs', 'VGPR'), ('NumAgprs', 'AGPR'), ('ScratchSize', 'scratch'), ('spill', 'spilled'), ('LDSByteSize', 'LDS'), ('Occupancy', 'occ'))


def demangle(names):
    try:
        out = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.split('\n')
        return {n: re.sub(r'^void |\(.*$|dir::\(anonymous namespace\)::|dir::convk::', '', d) for n, d in zip(names, out)}
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def parse(path):
    """{kernel symbol: (figures dict, Counter of mnemonics)}"""
    text = open(path).read()
    spills = dict(re.findall(r'\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)', text))
    kernels = {}
    for m in re.finditer(r'^(\w+):\s*; @\1\n(.*?)^; Kernel info:\n(.*?)^\s*\.(?:text|section)', text, re.S | re.M):
        name, body, info = m.groups()
        fig = {k: int(v) for k, v in re.findall(r'^; (\w+): (\d+)', info, re.M)}
        fig['spill'] = int(spills.get(name, 0))
        ops = collections.Counter(l.split()[0] for l in body.split('\n') if l.startswith('\t') and not l.lstrip().startswith(('.', ';')))
        if not all(f in fig for f, _ in FIGURES) or not ops:
            sys.exit('%s: kernel %s lacks a figure (%s) or has no instructions: the assembly format is not the one this tool parses' % (path, name, sorted(fig)))
        kernels[name] = (fig, ops)
    if not kernels or len(kernels) != len(re.findall(r'^\s*\.amdhsa_kernel\s', text, re.M)):
        sys.exit('%s: parsed %d kernels, the file declares %d (.amdhsa_kernel): the assembly format is not the one this tool parses'
                 % (path, len(kernels), len(re.findall(r'^\s*\.amdhsa_kernel\s', text, re.M))))
    return kernels


def pinned(ops):
    c = collections.Counter()
    for op, n in ops.items():
        for p in PINNED:
            if op.startswith(p):
                c[p] += n
                break
    return c


def table(paths):
    for path in paths:
        ks = parse(path)
        names = demangle(list(ks))
        print('# %s' % path.split('/')[-1])
        print('%-58s' % 'kernel' + ''.join('%8s' % t for _, t in FIGURES) + ''.join('%11s' % p for p in PINNED))
        for k in sorted(ks, key=lambda k: names[k]):
            fig, ops = ks[k]
            c = pinned(ops)
            print('%-58s' % names[k][:57] + ''.join('%8d' % fig.get(f, -1) for f, _ in FIGURES) + ''.join('%11d' % c[p] for p in PINNED))


def diff(a, b):
    ka, kb = parse(a), parse(b)
    names = demangle(list(ka))
    ok = set(ka) == set(kb)
    if not ok:
        print('kernel sets differ: only in %s %s, only in %s %s' % (a, sorted(set(ka) - set(kb)), b, sorted(set(kb) - set(ka))))
    for k in sorted(set(ka) & set(kb), key=lambda k: names[k]):
        (fa, oa), (fb, ob) = ka[k], kb[k]
        figs = ['%s %d -> %d' % (t, fa.get(f, -1), fb.get(f, -1)) for f, t in FIGURES if fa.get(f) != fb.get(f)]
        ops = ['%s %+d' % (op, ob[op] - oa[op]) for op in sorted(set(oa) | set(ob)) if oa[op] != ob[op]]
        bad = figs + [o for o in ops if o.startswith(PINNED)]
        ok = ok and not bad
        print('%-58s %s' % (names[k][:57], 'equal' if not figs and not ops else ('PINNED DIFFER: ' if bad else 'free to differ: ') + ', '.join(figs + ops)))
    return ok


if __name__ == '__main__':
    if sys.argv[1:2] == ['--diff']:
        sys.exit(0 if diff(sys.argv[2], sys.argv[3]) else 1)
    table(sys.argv[1:])
