#!/usr/bin/env python3
"""Size and instruction counts of the fused dense-block chain kernels' block loops.

    python tools/loopsize.py [-D MACRO[=V]]... [tu ...]      (default: every csrc/*.hip that includes rdb_chain_kernel.h)

Each translation unit is compiled device-only for gfx950 (the flags of __graft_entry__.build) and disassembled with
llvm-objdump.  For every rdb_chain_kernel instantiation in it one JSON object is printed (one per line):

    tu, kernel (demangled), kernel_bytes,
    loop_bytes, loop_insts        the block loop: the smallest span [target, branch] of a backward branch that holds
                                  every MFMA of the kernel (the tile loop around it holds the tile set-up as well)
    mfma, span_insts, per_mfma    MFMAs in the loop; instructions from the first to the last of them; their ratio
    opcodes                       instructions of the loop by mnemonic
    valu                          vector-ALU instructions of the loop that are no MFMA (`v_*`): with one wave per SIMD
                                  each takes an issue slot of its own next to the MFMA stream
    valu_in_segments              .. of them between two MFMAs that are at most 40 instructions apart
    valu_tail                     .. of them behind the last MFMA
    kernel_s_memrealtime, kernel_scratch   s_memrealtime / scratch_* instructions in the whole kernel
    sgpr_spill_count, vgpr_spill_count     from the kernel's metadata in the code object's notes

A size and count report only: nothing is compared or asserted here.
"""
import collections
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'esrganplus_amd', 'csrc')
ROCM = os.environ.get('ROCM_PATH', '/opt/rocm')
HIPCC = os.environ.get('HIPCC', os.path.join(ROCM, 'bin', 'hipcc'))
LLVM = os.path.join(ROCM, 'llvm', 'bin')

SYM = re.compile(r'^([0-9a-f]+) <(.+)>:\s*$')
INS = re.compile(r'^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):\s*((?:[0-9A-Fa-f]{8}\s*)+)(?:<.*>)?\s*$')


def disassemble(tu, defines, tmp):
    src = tu if os.path.exists(tu) else os.path.join(CSRC, tu if tu.endswith('.hip') else tu + '.hip')
    obj = os.path.join(tmp, os.path.basename(src)[:-4] + '.co')
    subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '--offload-device-only', '--no-gpu-bundle-output'] +
                          ['-D' + d for d in defines] + ['-c', src, '-o', obj], stderr=subprocess.DEVNULL)
    notes = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', obj], text=True, capture_output=True).stdout
    return subprocess.check_output([os.path.join(LLVM, 'llvm-objdump'), '-d', obj], text=True), notes


def spill_counts(notes):
    """{kernel symbol: {sgpr_spill_count, vgpr_spill_count}} from the AMDGPU metadata note (YAML, one map per kernel)"""
    out, cur = {}, {}
    for line in notes.split('\n'):
        if line.startswith('  - '):               # a new entry of amdhsa.kernels (its arguments are nested deeper)
            cur = {}
        m = re.match(r'^(?:    |  - )\.(symbol|sgpr_spill_count|vgpr_spill_count):\s*(\S+)\s*$', line)
        if not m:
            continue
        if m.group(1) == 'symbol':
            out[m.group(2)[:-3] if m.group(2).endswith('.kd') else m.group(2)] = cur
        else:
            cur[m.group(1)] = int(m.group(2))
    return out


def demangle(names):
    filt = next((f for f in (os.path.join(LLVM, 'llvm-cxxfilt'), shutil.which('llvm-cxxfilt'), shutil.which('c++filt'))
                 if f and os.path.exists(f)), None)
    if not names or not filt:
        return {}
    out = subprocess.run([filt] + names, text=True, capture_output=True).stdout.split('\n')
    return dict(zip(names, out))


def kernels(text):
    """{symbol: [(addr, bytes, mnemonic, operands)]}"""
    fns, cur = collections.OrderedDict(), None
    for line in text.split('\n'):
        m = SYM.match(line)
        if m:
            cur = fns.setdefault(m.group(2), [])
            continue
        m = INS.match(line)
        if m and cur is not None:
            cur.append((int(m.group(3), 16), 4 * len(m.group(4).split()), m.group(1), m.group(2)))
    return fns


def branch_target(addr, ops):
    m = re.match(r'^(\d+)', ops)
    if not m:
        return None
    off = int(m.group(1)) & 0xFFFF
    if off >= 0x8000:
        off -= 0x10000
    return addr + 4 + 4 * off


def is_valu(op):
    return op.startswith('v_') and not op.startswith('v_mfma')


def report(tu, name, pretty, ins, spills=None):
    r = collections.OrderedDict(tu=tu, kernel=pretty, kernel_bytes=sum(i[1] for i in ins))
    mf = [i[0] for i in ins if i[2].startswith('v_mfma')]
    best = None
    for a, _, op, ops in ins:
        if op == 's_branch' or op.startswith('s_cbranch'):
            t = branch_target(a, ops)
            if t is not None and t <= a and mf and t <= mf[0] and a >= mf[-1] and (best is None or a - t < best[1] - best[0]):
                best = (t, a)
    if best:
        loop = [i for i in ins if best[0] <= i[0] <= best[1]]
        span = [i for i in loop if mf[0] <= i[0] <= mf[-1]]
        r['loop_bytes'] = sum(i[1] for i in loop)
        r['loop_insts'] = len(loop)
        r['mfma'] = len(mf)
        r['span_insts'] = len(span)
        r['per_mfma'] = round(len(span) / len(mf), 3)
        r['opcodes'] = dict(collections.Counter(i[2] for i in loop).most_common())
        r['valu'] = sum(is_valu(i[2]) for i in loop)
        at = [k for k, i in enumerate(loop) if i[2].startswith('v_mfma')]
        r['valu_in_segments'] = sum(sum(is_valu(i[2]) for i in loop[a + 1:b]) for a, b in zip(at, at[1:]) if b - a - 1 <= 40)
        r['valu_tail'] = sum(is_valu(i[2]) for i in loop[at[-1] + 1:])
    else:
        r['loop_bytes'] = None
    r['kernel_s_memrealtime'] = sum(i[2] == 's_memrealtime' for i in ins)
    r['kernel_scratch'] = sum(i[2].startswith('scratch_') for i in ins)
    for k in ('sgpr_spill_count', 'vgpr_spill_count'):
        r[k] = (spills or {}).get(k)
    return r


def main(argv):
    defines, tus = [], []
    it = iter(argv)
    for a in it:
        if a == '-D':
            defines.append(next(it))
        elif a.startswith('-D'):
            defines.append(a[2:])
        else:
            tus.append(a)
    if not tus:
        tus = sorted(f for f in glob.glob(os.path.join(CSRC, '*.hip')) if '#include "rdb_chain_kernel.h"' in open(f).read())
    with tempfile.TemporaryDirectory() as tmp:
        for tu in tus:
            text, notes = disassemble(tu, defines, tmp)
            fns = kernels(text)
            spills = spill_counts(notes)
            names = [n for n in fns if 'rdb_chain_kernel' in n]
            pretty = demangle(names)
            for n in names:
                print(json.dumps(report(os.path.basename(tu).replace('.hip', ''), n, pretty.get(n, n), fns[n], spills.get(n))), flush=True)


if __name__ == '__main__':
    main(sys.argv[1:])
