"""CPU tests of the device-resident training set (esrganplus_amd.data: TrainSet, batch_reference, modcrop;
esr_batch_assemble's ABI): the symbol and its structs, the draw order, every constructor refusal — all before the device
is touched — and ``batch_reference``, the yardstick of tests/test_gpu_batch.py, against what the reference's own
``LRHRDataset.__getitem__`` returned (tests/golden/batch_assemble.npz, tools/gen_batch_golden.py)."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    from esrganplus_amd import _lib
    return _lib


def _u8(h, w, c=3, seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, c)).astype(np.uint8)


# ---- ABI -----------------------------------------------------------------------------------------------------------
def test_batch_assemble_is_exported_declared_and_abi_stays_6(built, tmp_path):
    hdr = os.path.join(ROOT, 'include', 'esrgan_hip.h')
    text = open(hdr).read()
    assert 'esr_batch_assemble' in built.EXPORTS
    assert re.search(r'^int esr_batch_assemble\(const esr_batch\* p, esr_stream_t stream\);', text, flags=re.M)
    L = built.lib()
    assert hasattr(L, 'esr_batch_assemble')
    assert L.esr_abi_version() == 6
    assert L.esr_sizeof_op() == ctypes.sizeof(built.esr_op)              # the entry point is no member of the op union
    assert 'batch' not in [f[0] for f in built._op_union._fields_]
    # struct sizes and every field offset as the host compiler lays the header out
    prints = []
    for n in ('esr_batch', 'esr_batch_item'):
        prints.append('printf("%s . %%zu\\n", sizeof(%s));' % (n, n))
        prints += ['printf("%s %s %%zu\\n", offsetof(%s, %s));' % (n, f[0], n, f[0]) for f in getattr(built, n)._fields_]
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){%s return 0;}\n' % (hdr, '\n'.join(prints)))
    subprocess.check_call(['gcc', '-std=c99', str(src), '-o', str(tmp_path / 'sz')])
    lines = subprocess.check_output([str(tmp_path / 'sz')]).decode().splitlines()
    assert len(lines) == len(prints)
    for line in lines:
        n, f, v = line.split()
        st = getattr(built, n)
        assert int(v) == (ctypes.sizeof(st) if f == '.' else getattr(st, f).offset), line
    # the record array TrainSet fills is that struct
    from esrganplus_amd import data as D
    assert D._item_dtype().itemsize == ctypes.sizeof(built.esr_batch_item)


def test_host_refusals_need_no_device(built):
    L = built.lib()
    assert L.esr_batch_assemble(None, None) == -1
    a = built.esr_batch()
    assert L.esr_batch_assemble(ctypes.byref(a), None) == -1 and b'esr_batch_assemble' in L.esr_last_error()


# ---- draw ----------------------------------------------------------------------------------------------------------
def _host_set(sizes, **kw):
    """A TrainSet's host half (what ``draw`` reads) without a device: the constructor's validation is what the refusal
    tests exercise; here only the sizes matter."""
    from esrganplus_amd import data as D
    ts = object.__new__(D.TrainSet)
    ts.scale, ts.lr_size = kw.get('scale', 4), kw.get('lr_size', 16)
    ts.use_flip, ts.use_rot = kw.get('use_flip', True), kw.get('use_rot', True)
    ts.sizes = list(sizes)
    ts.lr_sizes = [(h // ts.scale, w // ts.scale) for h, w in sizes]
    return ts


def test_draw_follows_the_reference_order_and_crop_and_augment():
    from esrganplus_amd import data as D
    sizes = [(80, 96), (96, 80), (160, 72)]
    ts = _host_set(sizes)
    ids = [0, 1, 2, 1, 0]
    random.seed(33)
    got = ts.draw(ids)
    random.seed(33)
    want = []
    for i in ids:
        h, w = sizes[i][0] // 4, sizes[i][1] // 4
        y0, x0 = random.randint(0, max(0, h - 16)), random.randint(0, max(0, w - 16))
        hf, vf, r9 = random.random() < 0.5, random.random() < 0.5, random.random() < 0.5
        want.append((y0, x0, int(hf) | int(vf) << 1 | int(r9) << 2))
    assert got == want and len({d[2] for d in got}) > 1
    # same-size inputs: the same consumption of `random` as crop_and_augment, and the same windows and flips
    ts = _host_set([(80, 96)] * 4)
    lr = torch.arange(4 * 3 * 20 * 24, dtype=torch.float32).reshape(4, 3, 20, 24)
    hr = torch.arange(4 * 3 * 80 * 96, dtype=torch.float32).reshape(4, 3, 80, 96)
    random.seed(5)
    draws = ts.draw(range(4))
    state = random.getstate()
    random.seed(5)
    cl, ch = D.crop_and_augment(lr, hr, 16, 4)
    assert random.getstate() == state
    rl, rh = D.batch_reference(list(hr), list(lr), 4, 16, draws)
    assert torch.equal(rl, cl) and torch.equal(rh, ch)


def test_draw_without_flips_consumes_two_randints():
    ts = _host_set([(80, 96), (96, 80)], use_flip=False, use_rot=False)
    random.seed(9)
    got = ts.draw([0, 1])
    random.seed(9)
    want = [(random.randint(0, 20 - 16), random.randint(0, 24 - 16), 0), (random.randint(0, 24 - 16), random.randint(0, 20 - 16), 0)]
    assert got == want
    assert random.getstate()[1] == _state_after(9, lambda: [random.randint(0, 4), random.randint(0, 8), random.randint(0, 8), random.randint(0, 4)])
    # hflip alone draws one coin per item, rot alone two
    for flip, rot, coins in ((True, False, 1), (False, True, 2)):
        ts = _host_set([(80, 96)], use_flip=flip, use_rot=rot)
        random.seed(4)
        (y0, x0, flags), = ts.draw([0])
        assert random.getstate()[1] == _state_after(4, lambda: [random.randint(0, 4), random.randint(0, 8)] + [random.random() for _ in range(coins)])
        assert flags & ~(1 if flip else 6) == 0


def _state_after(seed, fn):
    random.seed(seed)
    fn()
    return random.getstate()[1]


# ---- constructor refusals: ValueError on the host, before the device is touched -------------------------------------
def _refused(match, *a, **k):
    from esrganplus_amd import data as D
    with pytest.raises(ValueError, match=match):
        D.TrainSet(*a, **k)


def test_constructor_refusals_need_no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError('the device was touched before validation')
    monkeypatch.setattr(torch.cuda, 'current_device', touched)
    monkeypatch.setattr(torch.Tensor, 'to', touched)
    hr = [_u8(64, 80), _u8(96, 64, seed=1)]
    _refused('HR image 1 is 96 x 64, not 4 times its LR', hr, [_u8(16, 20), _u8(24, 17)], scale=4, lr_size=8)
    _refused('2 LR images for 1 HR', hr[:1], [_u8(16, 20), _u8(24, 16)], scale=4, lr_size=8)
    _refused('modcrop', [_u8(64, 80), _u8(66, 64)], scale=4, lr_size=8)                   # H no multiple of scale
    _refused('modcrop', [_u8(64, 81)], scale=4, lr_size=8)                                # W no multiple of scale
    _refused('modcrop', [_u8(64, 80)], scale=3, lr_size=8)
    _refused('smaller than the 32 x 32 window', hr, scale=4, lr_size=32)                  # generated LR 16 x 20
    _refused('smaller than the 18 x 18 window', hr, [_u8(16, 20), _u8(24, 16)], scale=4, lr_size=18)
    _refused('uint8 H x W x 3', [np.zeros((64, 80), dtype=np.uint8)], scale=4, lr_size=8)             # 2 dimensions
    _refused('uint8 H x W x 3', [_u8(64, 80, c=1)], scale=4, lr_size=8)                               # 1 channel
    _refused('uint8 H x W x 3', [_u8(64, 80).astype(np.float32)], scale=4, lr_size=8)                 # float HWC array
    _refused('float32 CHW tensor', [torch.zeros(1, 64, 80)], scale=4, lr_size=8)
    _refused('float32 CHW tensor', [torch.zeros(64, 80)], scale=4, lr_size=8)
    _refused('float32 CHW tensor', [torch.zeros(3, 64, 80, dtype=torch.float64)], scale=4, lr_size=8)
    _refused('one kind', [_u8(64, 80), torch.zeros(3, 64, 80)], scale=4, lr_size=8)
    _refused('one kind', [_u8(64, 80)], [torch.zeros(3, 16, 20)], scale=4, lr_size=8)
    _refused('scale must be one of', hr, scale=5, lr_size=8)
    _refused('lr_size must be', hr, scale=4, lr_size=0)
    _refused('no HR images', [], scale=4, lr_size=8)
    _refused('MI355X', hr, scale=4, lr_size=8, device='cpu')


def test_modcrop():
    from esrganplus_amd import data as D
    a = _u8(67, 81)
    m = D.modcrop(a, 4)
    assert m.shape == (64, 80, 3) and np.array_equal(m, a[:64, :80]) and not np.shares_memory(m, a)
    assert D.modcrop(a[:, :, 0], 3).shape == (66, 81)
    t = torch.arange(3 * 10 * 13.).reshape(3, 10, 13)
    assert torch.equal(D.modcrop(t, 4), t[:, :8, :12])
    assert D.modcrop(a[:64, :80], 4).shape == (64, 80, 3)
    with pytest.raises(ValueError):
        D.modcrop(np.zeros(5), 2)


# ---- batch_reference against the reference's dataset ----------------------------------------------------------------
def test_batch_reference_matches_the_reference_dataset(golden):
    """HR bit for bit in both modes, LR bit for bit where LR images are given, generated LR within 2e-6 — the gate
    tests/test_data_path.py applies to the same tables against the same reference function."""
    from esrganplus_amd import data as D
    g = golden('batch_assemble')
    imgs = [g['img%d' % k] for k in range(int(g['n_images']))]
    assert len({im.shape for im in imgs}) == len(imgs) and all(im.dtype == np.uint8 for im in imgs)
    ids, s = [int(i) for i in g['indices']], int(g['lr_size'])
    seen = set()
    for scale in (int(v) for v in g['scales']):
        for mode in ('given', 'gen'):
            tag = 'x%d_%s' % (scale, mode)
            draws = [tuple(int(v) for v in d) for d in g[tag + '_draws']]
            seen |= {d[2] for d in draws}
            lr_imgs = [imgs[i][::scale, ::scale] for i in ids] if mode == 'given' else None
            lr, hr = D.batch_reference([imgs[i] for i in ids], lr_imgs, scale, s, draws, bgr=True)
            assert lr.dtype == torch.float32 and tuple(hr.shape) == (len(ids), 3, s * scale, s * scale)
            assert np.array_equal(hr.numpy(), g[tag + '_HR']), tag
            d = float(np.abs(lr.numpy() - g[tag + '_LR']).max())
            print('%s: LR max difference to the reference %.3e' % (tag, d))
            if mode == 'given':
                assert np.array_equal(lr.numpy(), g[tag + '_LR']), tag
            else:
                assert d <= 2e-6, (tag, d)
    assert seen == set(range(8))                                          # the fixture meets every flip combination
