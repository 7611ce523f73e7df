"""Dev tool (CPU only): do two builds hold the same machine code?  Given two directories of hipcc -S listings (same file names,
e.g. one per source of build.SOURCES compiled with the build's flags plus --cuda-device-only -S at two commits), reports per
kernel symbol whether the instruction streams and the kernel descriptors (.amdhsa_* lines: registers, scratch, LDS) are
identical.  .file / .ident / .loc / __hip_cuid_* lines and comments are ignored.  For a kernel that differs: instruction counts,
the per-opcode histogram difference and the differing lines (-v: all of them, default the first 40).
usage: isa_diff.py <dir_a> <dir_b> [-v]      exit status 0 = every kernel identical, 1 = not."""
import collections, difflib, os, re, sys

SKIP = re.compile(r'^\s*\.(file|ident|loc|cfi_\w+|section|text|type|size|globl|protected|weak|hidden)\b|__hip_cuid_')


def clean(line):
    line = re.sub(r'\s*(;|//).*$', '', line).strip()
    return re.sub(r'\s+', ' ', line)


def kernels(path):
    """name -> (instruction and label lines of the body, .amdhsa_* lines of the descriptor)"""
    lines = open(path).read().split('\n')
    names = [m.group(1) for l in lines if (m := re.match(r'^\s*\.amdhsa_kernel\s+(\S+)', l))]
    out = {n: ([], []) for n in names}
    cur = desc = None
    for l in lines:
        if (m := re.match(r'^(\S+):', l)) and m.group(1) in out and not out[m.group(1)][0]:
            cur = m.group(1)
            continue
        if m := re.match(r'^\s*\.amdhsa_kernel\s+(\S+)', l):
            desc = m.group(1)
            continue
        if l.strip().startswith('.end_amdhsa_kernel'):
            desc = None
            continue
        if desc is not None:
            out[desc][1].append(clean(l))
            continue
        if cur is None:
            continue
        if re.match(r'^\.Lfunc_end\d+:', l):
            cur = None
            continue
        if SKIP.search(l):
            continue
        c = clean(l)
        if c:
            out[cur][0].append(c)
    return out


def opcode(l):
    return None if l.endswith(':') or l.startswith('.') else l.split(' ')[0]


def main():
    verbose = '-v' in sys.argv
    a_dir, b_dir = [a for a in sys.argv[1:] if a != '-v'][:2]
    files = sorted(set(f for f in os.listdir(a_dir) if f.endswith('.s')) | set(f for f in os.listdir(b_dir) if f.endswith('.s')))
    bad = 0
    for f in files:
        pa, pb = os.path.join(a_dir, f), os.path.join(b_dir, f)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f'{f}: only in {a_dir if os.path.exists(pa) else b_dir}')
            bad += 1
            continue
        ka, kb = kernels(pa), kernels(pb)
        same = 0
        for name in sorted(set(ka) | set(kb)):
            if name not in ka or name not in kb:
                print(f'{f}: {name}: only in {a_dir if name in ka else b_dir}')
                bad += 1
                continue
            (ia, da), (ib, db) = ka[name], kb[name]
            if ia == ib and da == db:
                same += 1
                continue
            bad += 1
            na, nb = sum(1 for l in ia if opcode(l)), sum(1 for l in ib if opcode(l))
            print(f'{f}: {name}: DIFFERENT  ({na} / {nb} instructions)')
            for l in difflib.unified_diff(da, db, 'descriptor a', 'descriptor b', lineterm='', n=0):
                print('     ', l)
            ha, hb = (collections.Counter(filter(None, map(opcode, i))) for i in (ia, ib))
            for op in sorted(set(ha) | set(hb)):
                if ha[op] != hb[op]:
                    print(f'      histogram {op}: {ha[op]} / {hb[op]}')
            diff = [l for l in difflib.unified_diff(ia, ib, 'a', 'b', lineterm='', n=0) if not l.startswith(('---', '+++', '@@'))]
            for l in diff if verbose else diff[:40]:
                print('     ', l)
            if not verbose and len(diff) > 40:
                print(f'      ... {len(diff) - 40} more differing lines (-v)')
        print(f'{f}: {same} of {len(set(ka) | set(kb))} kernels identical')
    print('IDENTICAL' if not bad else f'{bad} kernels differ')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
