"""data.TrainSet on the MI355X: one esr_batch_assemble launch per batch against ``data.batch_reference`` (the pure-torch
restatement, itself pinned to the reference's ``LRHRDataset`` by tests/test_batch_host.py), against an fp64 evaluation of
the resample tables where LR is generated, and against the reference's fixture; guard bands round every output; the
op's refusals; back-to-back calls; a ``PSNRStep`` fed by it; ``tools/train_folder.py``."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.0
BAND = 4096                      # floats on either side of an output


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _u8(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def _f32(h, w, seed):
    return torch.from_numpy(np.random.RandomState(seed).rand(3, h, w).astype(np.float32))


def _draws(ts, ids, flags=range(8)):
    """Per sample: the windows at the four corners and one in the interior, under all the given flag combinations."""
    out_ids, draws = [], []
    for i in ids:
        lh, lw = ts.lr_sizes[i]
        my, mx = lh - ts.lr_size, lw - ts.lr_size
        for (y0, x0) in ((0, 0), (0, mx), (my, 0), (my, mx), (my // 2 + (my > 1), mx // 3 + (mx > 2))):
            for f in flags:
                out_ids.append(i)
                draws.append((y0, x0, f))
    return out_ids, draws


def _guarded(ts, ids, draws, dev):
    """The op on outputs carved from the middle of sentinel-filled buffers -> (lr, hr) after checking that no sentinel
    survives inside and that the bands on both sides are untouched."""
    B, s = len(ids), ts.lr_size
    n_lr, n_hr = B * 3 * s * s, B * 3 * s * s * ts.scale ** 2
    buf = torch.full((3 * BAND + n_lr + n_hr,), SENTINEL, dtype=torch.float32, device=dev)
    lr = buf[BAND:BAND + n_lr].view(B, 3, s, s)
    hr = buf[2 * BAND + n_lr:2 * BAND + n_lr + n_hr].view(B, 3, s * ts.scale, s * ts.scale)
    ts._assemble(np.asarray(ids, dtype=np.int64), np.asarray(draws, dtype=np.int64), lr, hr)
    torch.cuda.synchronize()
    host = buf.cpu()
    assert (host[:BAND] == SENTINEL).all() and (host[BAND + n_lr:2 * BAND + n_lr] == SENTINEL).all()
    assert (host[2 * BAND + n_lr + n_hr:] == SENTINEL).all()
    lr, hr = lr.cpu(), hr.cpu()
    assert not (lr == SENTINEL).any() and not (hr == SENTINEL).any()
    return lr, hr


# ---- 1. uint8 -> float: a true division --------------------------------------------------------------------------------
@pytest.mark.parametrize('bgr', [True, False])
def test_uint8_conversion_is_numpys_division(dev, bgr):
    from esrganplus_amd import data as D
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    img = np.stack([v, 255 - v, (v.astype(np.int32) * 7 % 256).astype(np.uint8)], axis=2)      # all 256 values per channel
    assert all(len(set(img[:, :, c].reshape(-1).tolist())) == 256 for c in range(3))
    want = np.transpose(img.astype(np.float32) / np.float32(255), (2, 0, 1))
    if bgr:
        want = want[::-1]
    for lr_imgs in ([img], None):                     # the copy of a given LR image; at scale 1 the generated one is x * 1
        ts = D.TrainSet([img], lr_imgs, scale=1, lr_size=16, bgr=bgr, device=dev)
        lr, hr = ts.batch([0], draws=[(0, 0, 0)])
        assert np.array_equal(hr[0].cpu().numpy(), want) and np.array_equal(lr[0].cpu().numpy(), want)
    assert not np.array_equal(want, np.transpose(img.astype(np.float32) * np.float32(1 / 255), (2, 0, 1)))   # the shortcut differs


# ---- 2. the copy path, bit for bit -------------------------------------------------------------------------------------
COPY_SIZES = ((96, 120), (120, 96), (84, 108))        # multiples of 12; at scale 4 the LR side is >= 21


@pytest.mark.parametrize('kind', ['u8', 'f32'])
@pytest.mark.parametrize('lr_size', [8, 20])          # 20: across the 16-wide LR tile; its HR windows across the 32-wide tiles
@pytest.mark.parametrize('scale', [2, 3, 4])
def test_copy_path_bit_for_bit_with_guard_bands(dev, scale, lr_size, kind):
    from esrganplus_amd import data as D
    make = _u8 if kind == 'u8' else _f32
    hr_imgs = [make(h, w, 10 + k) for k, (h, w) in enumerate(COPY_SIZES)]
    lr_imgs = [make(h // scale, w // scale, 20 + k) for k, (h, w) in enumerate(COPY_SIZES)]
    bgr = kind == 'u8'
    ts = D.TrainSet(hr_imgs, lr_imgs, scale=scale, lr_size=lr_size, bgr=bgr, device=dev)
    assert ts.sizes == list(COPY_SIZES) and len(ts) == 3
    ids, draws = _draws(ts, [0, 1, 2])                # 3 images x 5 windows x 8 flag combinations, mixed sizes in one batch
    assert {d[2] for d in draws} == set(range(8))
    want_lr, want_hr = D.batch_reference([hr_imgs[i] for i in ids], [lr_imgs[i] for i in ids], scale, lr_size, draws, bgr=bgr)
    lr, hr = _guarded(ts, ids, draws, dev)
    assert torch.equal(hr, want_hr) and torch.equal(lr, want_lr)
    # and through the public call (fresh outputs)
    lr2, hr2 = ts.batch(ids, draws=draws)
    assert torch.equal(hr2.cpu(), want_hr) and torch.equal(lr2.cpu(), want_lr)


# ---- 3. the generated path against fp64 --------------------------------------------------------------------------------
GEN_SIZES = ((192, 168), (168, 216))                  # H != W, multiples of 24; at scale 8 the LR side is >= 21


@pytest.mark.parametrize('kind', ['u8', 'f32'])
@pytest.mark.parametrize('lr_size', [8, 20])
@pytest.mark.parametrize('scale', [2, 3, 4, 8])
def test_generated_lr_against_fp64_tables(dev, scale, lr_size, kind):
    """Gate: (taps_y + taps_x + 2) 2^-24 max_o sum|wy| max_o sum|wx| max|x| — the worst-case rounding of two fp32 dot
    products in sequence, computed from the tables.  The corner windows' footprints are mirrored at each border."""
    from esrganplus_amd import data as D
    make = _u8 if kind == 'u8' else _f32
    hr_imgs = [make(h, w, 30 + k) for k, (h, w) in enumerate(GEN_SIZES)]
    ts = D.TrainSet(hr_imgs, None, scale=scale, lr_size=lr_size, bgr=False, device=dev)
    ids, draws = _draws(ts, [0, 1], flags=(0, 7, 5, 2))
    lr, hr = _guarded(ts, ids, draws, dev)
    _, want_hr = D.batch_reference([hr_imgs[i] for i in ids], None, scale, lr_size, draws)
    assert torch.equal(hr, want_hr)
    whole64, gates, whole_dev = [], [], []
    for im in hr_imgs:
        x = im if kind == 'f32' else torch.from_numpy(np.transpose(im.astype(np.float32) / np.float32(255), (2, 0, 1)).copy())
        wh, ih, _ = D.resample_tables(x.shape[1], 1.0 / scale)
        ww, iw, _ = D.resample_tables(x.shape[2], 1.0 / scale)
        y = (x.double()[:, ih.long(), :] * wh.double()[None, :, :, None]).sum(2)
        whole64.append((y[:, :, iw.long()] * ww.double()[None, None, :, :]).sum(3))
        gates.append((wh.shape[1] + ww.shape[1] + 2) * 2.0 ** -24 * float(wh.abs().sum(1).max()) * float(ww.abs().sum(1).max())
                     * float(x.abs().max()))
        whole_dev.append(D.imresize(x.to(dev), 1.0 / scale).cpu())
    worst = ident = 0.0
    for b, (i, (y0, x0, f)) in enumerate(zip(ids, draws)):
        def aug(t):
            t = t[:, y0:y0 + lr_size, x0:x0 + lr_size]
            for bit, fn in ((1, lambda t: t.flip(-1)), (2, lambda t: t.flip(-2)), (4, lambda t: t.transpose(-1, -2))):
                if f & bit:
                    t = fn(t)
            return t
        err = float((lr[b].double() - aug(whole64[i])).abs().max())
        worst = max(worst, err / gates[i])
        ident = max(ident, float((lr[b] - aug(whole_dev[i])).abs().max()))
        assert err <= gates[i], (b, i, (y0, x0, f), err, gates[i])
    print('x%d s=%d %s: worst error / gate %.3f (gates %s); max difference to data.imresize + crop %.3e (%s)'
          % (scale, lr_size, kind, worst, ['%.2e' % g for g in gates], ident, 'bit-identical' if ident == 0.0 else 'not bit-identical'))


# ---- 4. the reference's fixture through TrainSet.batch ------------------------------------------------------------------
def test_fixture_of_the_reference_dataset(dev, golden):
    from esrganplus_amd import data as D
    g = golden('batch_assemble')
    imgs = [g['img%d' % k] for k in range(int(g['n_images']))]
    ids, s = [int(i) for i in g['indices']], int(g['lr_size'])
    for scale in (int(v) for v in g['scales']):
        for mode in ('given', 'gen'):
            tag = 'x%d_%s' % (scale, mode)
            ts = D.TrainSet(imgs, [im[::scale, ::scale] for im in imgs] if mode == 'given' else None, scale=scale, lr_size=s,
                            bgr=True, device=dev)
            lr, hr = ts.batch(ids, draws=[tuple(int(v) for v in d) for d in g[tag + '_draws']])
            assert np.array_equal(hr.cpu().numpy(), g[tag + '_HR']), tag
            d = float(np.abs(lr.cpu().numpy() - g[tag + '_LR']).max())
            print('%s: LR max difference to the reference %.3e' % (tag, d))
            if mode == 'given':
                assert np.array_equal(lr.cpu().numpy(), g[tag + '_LR']), tag
            else:
                assert d <= 2e-6, (tag, d)


# ---- 5. back to back ----------------------------------------------------------------------------------------------------
def test_back_to_back_calls_without_synchronisation(dev):
    from esrganplus_amd import data as D
    hr_imgs = [_u8(h, w, 40 + k) for k, (h, w) in enumerate(COPY_SIZES)]
    lr_imgs = [_u8(h // 4, w // 4, 50 + k) for k, (h, w) in enumerate(COPY_SIZES)]
    ts = D.TrainSet(hr_imgs, lr_imgs, scale=4, lr_size=16, device=dev)
    random.seed(77)
    calls = []
    for k in range(D.TrainSet.RING + 2):              # more calls than pinned tables: the ring goes round once
        ids = [(k + j) % 3 for j in range(5)]
        calls.append((ids, ts.draw(ids)))
    assert len({tuple(c[1]) for c in calls}) == len(calls)
    torch.cuda.synchronize()
    outs = [ts.batch(ids, draws=draws) for ids, draws in calls]          # nothing synchronises in between
    torch.cuda.synchronize()
    assert len({o[0].data_ptr() for o in outs}) == len(outs)            # fresh outputs every call
    for (ids, draws), (lr, hr) in zip(calls, outs):
        want_lr, want_hr = D.batch_reference([hr_imgs[i] for i in ids], [lr_imgs[i] for i in ids], 4, 16, draws)
        assert torch.equal(lr.cpu(), want_lr) and torch.equal(hr.cpu(), want_hr)


def test_epoch_covers_the_set(dev):
    from esrganplus_amd import data as D
    ts = D.TrainSet([_u8(48, 48, k) for k in range(5)], None, scale=2, lr_size=8, device=dev)
    torch.manual_seed(3)
    got = list(ts.epoch(2))
    assert len(got) == 2 and all(tuple(l.shape) == (2, 3, 8, 8) and tuple(h.shape) == (2, 3, 16, 16) for l, h in got)
    assert len(list(ts.epoch(2, shuffle=False, drop_last=False))) == 3
    with pytest.raises(ValueError):
        ts.batch([0], draws=[(17, 0, 0)])             # a window outside its 24 x 24 LR image never reaches the device
    with pytest.raises(ValueError):
        ts.batch([5])


# ---- 6. feeds a step ----------------------------------------------------------------------------------------------------
def test_feeds_a_psnr_step_like_crop_and_augment(dev):
    from esrganplus_amd import architecture as arch, data as D, synth, train
    hr_pool = torch.stack([_f32(96, 112, 60 + k) for k in range(4)])
    lr_pool = torch.stack([_f32(24, 28, 70 + k) for k in range(4)])
    ts = D.TrainSet(list(hr_pool), list(lr_pool), scale=4, lr_size=16, device=dev)
    random.seed(123)
    lr, hr = ts.batch(range(4))
    random.seed(123)
    lr2, hr2 = D.crop_and_augment(lr_pool.to(dev), hr_pool.to(dev), 16, 4)
    assert torch.equal(lr, lr2) and torch.equal(hr, hr2)
    losses = []
    for a, b in ((lr, hr), (lr2.contiguous(), hr2.contiguous())):
        netG = arch.RRDBNet(3, 3, 64, 1).to(dev).train().set_precision('fp32')
        netG.load_state_dict(synth.rrdbnet_state_dict(nb=1, seed=7), strict=True)
        st = train.PSNRStep(netG)
        torch.manual_seed(900)                        # the Philox seeds of the noise layers come from torch's generator
        losses.append(st.step(a, b)['l_pix'])
        st.finish()
    assert np.isfinite(losses[0]) and losses[0] == losses[1], losses


# ---- 7. the op's refusals -------------------------------------------------------------------------------------------------
def test_op_refusals_launch_nothing(dev):
    from esrganplus_amd import data as D, _lib as L
    ts = D.TrainSet([_u8(48, 48, 80)], None, scale=2, lr_size=8, device=dev)
    lr = torch.full((1, 3, 8, 8), SENTINEL, device=dev)
    hr = torch.full((1, 3, 16, 16), SENTINEL, device=dev)
    good, table = ts._assemble(np.array([0]), np.array([[0, 0, 0]]), lr, hr)
    torch.cuda.synchronize()
    assert not (lr == SENTINEL).any() and not (hr == SENTINEL).any()
    lr.fill_(SENTINEL)
    hr.fill_(SENTINEL)
    lib = L.lib()

    def rc(**kw):
        a = L.esr_batch()
        C.memmove(C.addressof(a), C.addressof(good), C.sizeof(a))
        for k, v in kw.items():
            setattr(a, k, v)
        r = lib.esr_batch_assemble(C.byref(a), None)
        msg = lib.esr_last_error()
        assert b'esr_batch_assemble' in msg, (kw, msg)
        return r

    INVALID, UNSUPPORTED = -1, -3
    assert lib.esr_batch_assemble(None, None) == INVALID and b'esr_batch_assemble' in lib.esr_last_error()
    for kw in ({'items': None}, {'lr_out': None}, {'hr_out': None}, {'B': 0}, {'B': -3}, {'lr_size': 0}, {'scale': 5},
               {'scale': 0}, {'scale': 6}, {'src_format': 2}, {'src_format': -1}):
        assert rc(**kw) == INVALID, kw
    assert rc(C=4) == UNSUPPORTED and rc(C=1) == UNSUPPORTED
    assert rc(B=65536) == UNSUPPORTED
    assert rc(lr_size=1 << 21, scale=1) == UNSUPPORTED              # 2^32 tiles: over the grid's x limit
    assert rc(lr_size=1 << 30, scale=8) == UNSUPPORTED              # an HR side beyond int32
    torch.cuda.synchronize()
    assert (lr == SENTINEL).all() and (hr == SENTINEL).all()
    del table


# ---- 8. the tool ------------------------------------------------------------------------------------------------------------
def test_train_folder_tool_runs(tmp_path, golden):
    from PIL import Image
    from esrganplus_amd import data as D
    g = golden('sr_infer')
    hr_dir = tmp_path / 'HR'
    hr_dir.mkdir()
    for name in ('bird', 'butterfly', 'head', 'woman'):
        Image.fromarray(D.modcrop(g['sr_' + name], 4)).save(str(hr_dir / (name + '.png')))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train_folder.py'), str(hr_dir), '--nb', '1', '--batch', '4',
                        '--lr-size', '16', '--iters', '3'], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    losses = [float(line.split()[-1]) for line in r.stdout.splitlines() if line.startswith('iter ')]
    assert len(losses) == 3 and all(np.isfinite(v) for v in losses), r.stdout
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith('iters 3, last loss ') and float(last.split()[-1]) == pytest.approx(losses[-1], abs=1e-6)
