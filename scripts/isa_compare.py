"""The comparing half of scripts/isa_compare.sh:  isa_compare.py OUT a.hip b.hip ...  reads OUT/a/<stem>.s and OUT/b/<stem>.s.
An argument  a.hip=b.hip+c.hip  compares a file that tree B has split: the B side is the union of OUT/b/b.s and OUT/b/c.s.
Kernels are compared as ever; data objects and the remaining lines follow the sections of a file, so for a split file their
differences are printed and do not fail the run."""
import re
import sys

LOCAL = re.compile(r'\.L(BB|func_begin|func_end|tmp|JTI|CPI)\d+')
CUID = re.compile(r'__hip_cuid_[0-9a-f]+')
TYPE = re.compile(r'\.type\s+([^,\s]+),@(function|object)')


def parse(path):
    """-> {function: [instructions, descriptor, metadata]}, set of kernel names, {data object: lines}, other lines"""
    funcs, kernels, objects, other, is_func = {}, set(), {}, [], set()
    parts = lambda name: funcs.setdefault(name, [[], [], []])
    cur = desc = entry = obj = None      # function / descriptor / metadata entry / data object being read
    section = ''
    meta, key = False, ''

    def close_entry():
        name = next((l.split(':', 1)[1].strip() for l in entry if l.strip().startswith('.name:')), '?')
        parts(name)[2] = entry
        kernels.add(name)

    for raw in open(path, errors='replace'):
        if meta:                   # the amdgpu_metadata note (YAML): one "  - " item of amdhsa.kernels per kernel
            line = CUID.sub('__hip_cuid', raw.rstrip())
            item = key == 'amdhsa.kernels:' and line.startswith('  - ')
            if entry is not None and (item or not line.startswith('   ')):
                close_entry()
                entry = None
            if item:
                entry = [line]
            elif entry is not None:
                entry.append(line)
            else:
                if line and not line[0].isspace():
                    key = line.strip()
                meta = '.end_amdgpu_metadata' not in line
                other.append(line)
            continue
        line = CUID.sub('__hip_cuid', LOCAL.sub(lambda m: '.L' + m.group(1), raw.split(';', 1)[0])).strip()
        if not line:
            continue
        if line.startswith('.amdgpu_metadata'):
            meta = True
            other.append(line)
        elif line.startswith('.amdhsa_kernel '):
            desc = line.split()[1]
            kernels.add(desc)
            parts(desc)[1].append(line)
        elif desc is not None:
            parts(desc)[1].append(line)
            if line == '.end_amdhsa_kernel':
                desc = None
        elif cur is None and line.endswith(':') and line[:-1] in is_func:
            cur = line[:-1]
            parts(cur)[0].append(line)
        elif cur is not None:
            parts(cur)[0].append(line)
            if line.startswith('.Lfunc_end'):
                cur = None
        elif line.startswith('.section') or line in ('.text', '.data', '.bss'):
            section = line         # (kept with each data object: in which order the compiler emits those is an accident)
            if obj is not None:    # (the first object of a section names it after its own .type line)
                objects[obj][0] = line
        elif obj is not None:
            objects[obj].append(line)
            if line.startswith('.size'):
                obj = None
        else:
            m = TYPE.match(line)
            if m and m.group(2) == 'function':
                is_func.add(m.group(1))
            if m and m.group(2) == 'object':
                obj = m.group(1)
                objects[obj] = [section, line]
            elif line.startswith('.addrsig_sym'):
                objects.setdefault('.addrsig', []).append(line)      # (one per data object, in their order)
            else:
                other.append(line)
    objects.get('.addrsig', []).sort()
    return funcs, kernels, objects, other


PART = ('instructions', 'descriptor', 'metadata')
USE = re.compile(r'\.(vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size|private_segment_fixed_size):\s*(\d+)')


def resources(parts):
    """What a kernel uses, for the report of one that differs: instruction count + the register / spill / LDS / scratch metadata."""
    use = {'instructions': sum(1 for l in parts[0] if not l.endswith(':') and not l.startswith('.'))}
    use.update((m.group(1), int(m.group(2))) for m in map(USE.search, parts[2]) if m)
    return use


out, srcs = sys.argv[1], sys.argv[2:]
bad, total = 0, [0, 0]
for src in srcs:
    src, _, split = src.partition('=')
    fa, ka, da, oa = parse(f'{out}/a/{src[:-4]}.s')
    fb, kb, db, ob = {}, set(), {}, []
    for part in (split or src).split('+'):
        f, k, d, o = parse(f'{out}/b/{part[:-4]}.s')
        fb.update(f), kb.update(k), db.update(d), ob.extend(o)
    diffs, soft = [], []
    for name in sorted(set(fa) | set(fb)):
        if name not in fa or name not in fb:
            diffs.append(f'{name} (only in {"A" if name in fa else "B"})')
            continue
        which = [part for i, part in enumerate(PART) if fa[name][i] != fb[name][i]]
        if which:
            ra, rb = resources(fa[name]), resources(fb[name])
            diffs.append(f'{name} ({", ".join(which)}): ' + ', '.join(f'{k} {ra[k]} -> {rb.get(k)}' for k in ra))
    (soft if split else diffs).extend(f'{name} (data object)' for name in sorted(set(da) | set(db)) if da.get(name) != db.get(name))
    if oa != ob:
        (soft if split else diffs).append('<other>')
    total[0] += len(ka)
    total[1] += len(kb)
    print(f'{src:18s} kernels {len(ka):4d} / {len(kb):4d}  other functions {len(fa) - len(ka):2d} / {len(fb) - len(kb):2d}  '
          + ('identical' if not diffs else f'{len(diffs)} differences'))
    for d in diffs:
        print(f'    differs: {d}')
    for d in soft:
        print(f'    differs (split file, not counted): {d}')
    bad += bool(diffs)
print(f'{"total":18s} kernels {total[0]:4d} / {total[1]:4d}  ' + ('identical' if not bad else f'{bad} file(s) differ'))
sys.exit(1 if bad else 0)
