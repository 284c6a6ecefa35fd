#!/usr/bin/env python3
"""Build check for refactors that must not touch device code: the gfx950 kernels of HIP translation units, kernel by kernel.

    python scripts/kernel_isa_table.py dump OUT.json FILE.hip [FILE.hip ...] [-- extra hipcc flags, e.g. -DPVHIP_DIAG]
    python scripts/kernel_isa_table.py compare BEFORE.json AFTER.json        # markdown table on stdout, exit 1 on a difference

`dump` compiles the device side of each file with the flags of csrc/Makefile (hipcc --cuda-device-only), unbundles the gfx950 code
object and records per kernel -- keyed by the demangled name with namespaces stripped -- the number of instruction encoding words, a
sha1 over their sequence (llvm-objdump -d, the hex column only) and the resource metadata (llvm-readelf --notes).  A kernel that
several of the files instantiate is recorded once if the copies are identical and is an error otherwise.  Needs no GPU.
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get('ROCM_PATH', '/opt/rocm')
LLVM = os.path.join(ROCM, 'lib', 'llvm', 'bin')
CXXFLAGS = '-O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function --offload-arch=gfx950'.split()
META = ('.vgpr_count', '.sgpr_count', '.agpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size', '.kernarg_segment_size')


def run(cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout


def plain(names):
    """demangled, without namespaces and without the return type"""
    out = run(['c++filt'] + names).splitlines()
    return [re.sub(r'^void ', '', re.sub(r'\(anonymous namespace\)::|pvhip::', '', n)) for n in out]


def kernels_of(path, flags):
    with tempfile.TemporaryDirectory() as tmp:
        bundle, elf = os.path.join(tmp, 'k.bundle'), os.path.join(tmp, 'k.elf')
        subprocess.run([os.path.join(ROCM, 'bin', 'hipcc')] + CXXFLAGS + flags + ['--cuda-device-only', '-c', path, '-o', bundle], check=True)
        subprocess.run([os.path.join(LLVM, 'clang-offload-bundler'), '--unbundle', '--type=o', '--input=' + bundle,
                        '--targets=hip-amdgcn-amd-amdhsa--gfx950', '--output=' + elf], check=True)
        notes = run([os.path.join(LLVM, 'llvm-readelf'), '--notes', elf])
        asm = run([os.path.join(LLVM, 'llvm-objdump'), '-d', elf])
    # amdhsa.kernels: one record per kernel, '  - .key: value' opens it, its own keys are indented by four spaces
    records = []
    for line in notes.splitlines():
        m = re.match(r'^  (-| ) (\.[a-z_]+):\s*(.*)$', line)
        if not m:
            continue
        if m.group(1) == '-':
            records.append({})
        if records:
            records[-1][m.group(2)] = m.group(3).strip().strip("'")
    meta = {r['.symbol'][:-3]: {k: int(r[k]) for k in META if k in r} for r in records if r.get('.symbol', '').endswith('.kd')}
    words, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
        if m:
            cur = m.group(1)
            words[cur] = []
            continue
        m = re.search(r'//\s*[0-9A-F]+:\s*((?:[0-9A-F]{8}\s*)+)$', line)
        if m and cur is not None:
            words[cur] += m.group(1).split()
    names = sorted(meta)
    assert names and all(words.get(n) for n in names), 'kernel metadata without code in ' + path
    out = {}
    for n, p in zip(names, plain(names)):
        out[p] = {'words': len(words[n]), 'sha1': hashlib.sha1(' '.join(words[n]).encode()).hexdigest()[:16], 'meta': meta[n]}
    return out


def dump(out_path, files, flags):
    table = {}
    for f in files:
        for k, v in kernels_of(f, flags).items():
            assert table.get(k, v) == v, 'two different copies of ' + k
            table[k] = v
    with open(out_path, 'w') as fh:
        json.dump(table, fh, indent=1, sort_keys=True)
    print(len(table), 'kernels ->', out_path)


def compare(before, after):
    a, b = json.load(open(before)), json.load(open(after))
    bad = 0
    print('| kernel | words | vgpr / sgpr / agpr | LDS | scratch | kernarg | |')
    print('|---|---|---|---|---|---|---|')
    for k in sorted(set(a) | set(b)):
        ref = a.get(k) or b[k]
        m = ref['meta']
        same = k in a and k in b and all(a[k][f] == b[k][f] for f in ('words', 'sha1', 'meta'))
        verdict = 'equal' if same else ('removed' if k not in b else ('ADDED' if k not in a else 'DIFFERENT'))
        bad += verdict in ('ADDED', 'DIFFERENT')
        print('| `{}` | {} | {} / {} / {} | {} | {} | {} | {} |'.format(
            k, ref['words'], m.get('.vgpr_count'), m.get('.sgpr_count'), m.get('.agpr_count'), m.get('.group_segment_fixed_size'),
            m.get('.private_segment_fixed_size'), m.get('.kernarg_segment_size'), verdict))
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) >= 4 and sys.argv[1] == 'dump':
        rest = sys.argv[3:]
        cut = rest.index('--') if '--' in rest else len(rest)
        dump(sys.argv[2], rest[:cut], rest[cut + 1:])
    elif len(sys.argv) == 4 and sys.argv[1] == 'compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
