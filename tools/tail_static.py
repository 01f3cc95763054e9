#!/usr/bin/env python3
"""Static figures of the conv_kernel instantiations of csrc/conv_mfma.hip (the launches around the fused chain: head,
up-convs, HR tail): how much code stands in front of and behind the K loop's MFMAs, and what the register allocator did.

    python tools/tail_static.py [--src FILE] [--all] [-D MACRO[=V]]... > profiles/<name>.json

The translation unit (default csrc/conv_mfma.hip; --src compiles another revision of it against the headers of this
tree) is compiled device-only for gfx950 with the flags of __graft_entry__.build and disassembled (tools/loopsize.py
does the same for the chain).  One JSON object per kernel, one per line:

    kernel, dtype and the template arguments by name (plain: the PLAIN argument), insts, mfma,
    pre, post                instructions in front of the first / behind the last MFMA of the kernel, each split by
                             mnemonic prefix: valu (v_*), salu (s_*), lds (ds_*), vmem (global_* / buffer_*),
                             scratch (scratch_*), other
    whole                    the same split over the whole kernel
    sgpr_spill_count, vgpr_spill_count, scratch_bytes (.private_segment_fixed_size), vgpr_count, sgpr_count

Without --all only the fp16 forward kernels the x4 forward's tail runs are listed: 3x3/s1 on 16-row tiles with one and
two cout blocks per wave (plain K loop) and the sub-pixel up-conv with two, general and plain.  A report only: nothing
is compared or asserted here."""
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loopsize as LS  # noqa: E402

KEYS = ('ks', 's', 'ups', 'wr', 'wc', 'ncg', 'ncw', 'wlds', 'has1x1', 'bwd', 'pipe', 'rw', 'pack', 'plain')
# the x4 forward's tail: ks, s, ups, wr, wc, ncg, ncw of its three kernels (fp16, forward, plain K loop, 16-row tiles)
TAIL = {(3, 1, 0, 4, 1, 1, 1), (3, 1, 0, 4, 1, 1, 2), (2, 1, 3, 2, 1, 4, 2)}


def template_args(symbol):
    """('f16' | 'f32', {ks, s, ..., plain}) of a conv_kernel instantiation, from its mangled name (defaults filled in)"""
    m = re.search(r'conv_kernelI(DF16_|f)((?:L[ib]\d+E)+)', symbol)
    if not m:
        return None, {}
    v = [int(x) for x in re.findall(r'L[ib](\d+)E', m.group(2))]
    v += [0, 4, 0, 0][len(v) - 10:] if len(v) < 14 else []
    return ('f32' if m.group(1) == 'f' else 'f16'), collections.OrderedDict(zip(KEYS, v))


def metadata(notes):
    """{kernel symbol: {field: int}} from the AMDGPU metadata note"""
    out, cur = {}, {}
    for line in notes.split('\n'):
        if line.startswith('  - '):
            cur = {}
        m = re.match(r'^(?:    |  - )\.(symbol|sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size|vgpr_count|sgpr_count):'
                     r'\s*(\S+)\s*$', line)
        if not m:
            continue
        if m.group(1) == 'symbol':
            out[m.group(2)[:-3] if m.group(2).endswith('.kd') else m.group(2)] = cur
        else:
            cur[m.group(1)] = int(m.group(2))
    return out


def split(ins):
    c = collections.OrderedDict(insts=len(ins), valu=0, salu=0, lds=0, vmem=0, scratch=0, other=0)
    for _, _, op, _ in ins:
        if op.startswith('v_mfma'):
            k = 'other'
        elif op.startswith('v_'):
            k = 'valu'
        elif op.startswith('s_'):
            k = 'salu'
        elif op.startswith('ds_'):
            k = 'lds'
        elif op.startswith('global_') or op.startswith('buffer_'):
            k = 'vmem'
        elif op.startswith('scratch_'):
            k = 'scratch'
        else:
            k = 'other'
        c[k] += 1
    return c


def report(symbol, ins, md):
    at = [k for k, i in enumerate(ins) if i[2].startswith('v_mfma')]
    dt, a = template_args(symbol)
    r = collections.OrderedDict(kernel='conv_kernel<%s, %s>' % (dt, ', '.join(str(x) for x in a.values())), dtype=dt)
    r.update(a)
    r['insts'], r['mfma'] = len(ins), len(at)
    r['pre'] = split(ins[:at[0]]) if at else None
    r['post'] = split(ins[at[-1] + 1:]) if at else None
    r['whole'] = split(ins)
    r['sgpr_spill_count'] = md.get('sgpr_spill_count')
    r['vgpr_spill_count'] = md.get('vgpr_spill_count')
    r['scratch_bytes'] = md.get('private_segment_fixed_size')
    r['vgpr_count'], r['sgpr_count'] = md.get('vgpr_count'), md.get('sgpr_count')
    return r


def main(argv):
    src, every, defines = os.path.join(LS.CSRC, 'conv_mfma.hip'), False, []
    it = iter(argv)
    for a in it:
        if a == '--src':
            src = next(it)
        elif a == '--all':
            every = True
        elif a == '-D':
            defines.append(next(it))
        elif a.startswith('-D'):
            defines.append(a[2:])
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, 'conv.co')
        subprocess.check_call([LS.HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '--offload-device-only',
                               '--no-gpu-bundle-output', '-x', 'hip', '-I', LS.CSRC, '-I', os.path.join(LS.ROOT, 'include')] +
                              ['-D' + d for d in defines] + ['-c', src, '-o', obj], stderr=subprocess.DEVNULL)
        notes = subprocess.run([os.path.join(LS.LLVM, 'llvm-readelf'), '--notes', obj], text=True, capture_output=True).stdout
        text = subprocess.check_output([os.path.join(LS.LLVM, 'llvm-objdump'), '-d', obj], text=True)
    fns, md = LS.kernels(text), metadata(notes)
    for n in fns:
        dt, a = template_args(n)
        if dt is None:
            continue
        tail = dt == 'f16' and tuple(a.values())[:7] in TAIL and not (a['has1x1'] or a['bwd'] or a['pipe'] or a['pack']) and a['rw'] == 4
        if every or tail:
            print(json.dumps(report(n, fns[n], md.get(n, {}))), flush=True)


if __name__ == '__main__':
    main(sys.argv[1:])
