#!/usr/bin/env python
"""Inference harness reproducing the reference's ``test_image/test.py`` (lines 9-40) on the HIP path
with PIL instead of cv2:  python tools/sr_infer.py <model.pth|synthetic> <in_dir> <out_dir> [fp16|fp32] [--scale S] [--x8] [--tile N[,PAD]] [--tile-x8 N[,PAD]] [--tile-many N[,PAD]] [--tile-u8 N[,PAD]] [--tile-many-x8 N[,PAD]] [--tile-u8-x8 N[,PAD]]

Per image: RGB /255 -> NCHW float32 -> RRDB_Net(3,3,64,23,...) -> clamp(0,1) -> *255 round -> PNG.
--scale S (also --scale=S; 1, 2, 3, 4 or 8, default 4): the ``upscale`` the network is built with.
--x8: the geometric self-ensemble (the reference's ``SRModel.test_x8``, codes/models/SR_model.py:82-120) in place of the
plain forward: ``model.forward_x8``.
--tile N[,PAD] (also --tile=N[,PAD]): the tiled forward ``model.forward_tiled(x, tile=N, pad=PAD)`` (PAD defaults to the
method's): one launch plan for a folder of images of any size, bounded memory; not combined with --x8.
--tile-x8 N[,PAD] (also --tile-x8=N[,PAD]): the tiled self-ensemble ``model.forward_tiled_x8(x, tile=N, pad=PAD)``: the
ensemble per window, with the tiled forward's bounded memory and shared plan; not combined with --x8 or --tile.
--tile-many N[,PAD] (also --tile-many=N[,PAD]): the tiled forward over the folder,
``model.forward_tiled_many(images, tile=N, pad=PAD)``: the windows of different images share the passes, so small and
odd-sized images run at the cost of full passes.  Images are queued until they hold at least 4 x 16 windows (or the
folder ends), run in one call and written; the output of each image is that of the call it ran in.  Not combined with
--x8, --tile or --tile-x8.
--tile-u8 N[,PAD] (also --tile-u8=N[,PAD]): --tile-many's folder queueing through
``model.forward_images(images, tile=N, pad=PAD)``: the 8-bit image goes to the device as it is and the 8-bit result comes
back, the / 255 and the clamp, x 255, round run inside the gather and stitch kernels — the same arithmetic, no per-pixel
numpy.  N >= the largest image side runs every image whole.  Not combined with --x8, --tile, --tile-x8 or --tile-many.
--tile-many-x8 N[,PAD] / --tile-u8-x8 N[,PAD] (also with =): --tile-many / --tile-u8 with the x8 self-ensemble per window,
``model.forward_tiled_many_x8(images, tile=N, pad=PAD)`` / ``model.forward_images(images, tile=N, pad=PAD, x8=True)``: the
reference's best-quality result for a folder, the windows of different images sharing the passes.  Each by itself.
The tiled forms are x4-only: with another --scale the script exits with the library's message."""
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image

from esrganplus_amd import architecture as arch, synth


def main():
    argv = [a for a in sys.argv[1:] if a != '--x8']
    x8 = '--x8' in sys.argv[1:]
    tiles = {'--tile': None, '--tile-x8': None, '--tile-many': None, '--tile-u8': None, '--tile-many-x8': None,
             '--tile-u8-x8': None}
    for flag in tiles:
        for i, a in enumerate(argv):
            if a == flag or a.startswith(flag + '='):
                val = a[len(flag) + 1:] if '=' in a else ''.join(argv[i + 1:i + 2])
                del argv[i:i + (1 if '=' in a else 2)]
                try:
                    tiles[flag] = [int(v) for v in val.split(',')]
                except ValueError:
                    tiles[flag] = []
                if len(tiles[flag]) not in (1, 2):
                    sys.exit('sr_infer.py: %s takes N or N,PAD (LR pixels), got %r' % (flag, val))
                break
    tiled, tiled_x8, tiled_many, tiled_u8 = tiles['--tile'], tiles['--tile-x8'], tiles['--tile-many'], tiles['--tile-u8']
    scale = 4
    for i, a in enumerate(argv):
        if a == '--scale' or a.startswith('--scale='):
            val = a[len('--scale='):] if '=' in a else ''.join(argv[i + 1:i + 2])
            del argv[i:i + (1 if '=' in a else 2)]
            if val not in ('1', '2', '3', '4', '8'):
                sys.exit('sr_infer.py: --scale takes 1, 2, 3, 4 or 8, got %r' % val)
            scale = int(val)
            break
    if tiled and x8:
        sys.exit('sr_infer.py: --tile and --x8 cannot be combined: the tiled self-ensemble is --tile-x8 N[,PAD]')
    if tiled_x8 and (x8 or tiled):
        sys.exit('sr_infer.py: --tile-x8 is the tiled self-ensemble by itself: it cannot be combined with --x8 or --tile')
    if tiled_many and (x8 or tiled or tiled_x8):
        sys.exit('sr_infer.py: --tile-many is the tiled forward over the folder by itself: it cannot be combined with '
                 '--x8, --tile or --tile-x8')
    if tiled_u8 and (x8 or tiled or tiled_x8 or tiled_many):
        sys.exit('sr_infer.py: --tile-u8 is the 8-bit tiled forward over the folder by itself: it cannot be combined with '
                 '--x8, --tile, --tile-x8 or --tile-many')
    for flag in ('--tile-many-x8', '--tile-u8-x8'):
        if tiles[flag] and (x8 or sum(v is not None for v in tiles.values()) > 1):
            sys.exit('sr_infer.py: %s is the self-ensemble over the folder by itself: it cannot be combined with --x8 or '
                     'another --tile form' % flag)
    set_x8 = tiles['--tile-many-x8'] or tiles['--tile-u8-x8']
    model_path, in_dir, out_dir = argv[0], argv[1], argv[2]
    prec = argv[3] if len(argv) > 3 else 'fp32'
    dev = torch.device('cuda')
    model = arch.RRDB_Net(3, 3, 64, 23, gc=32, upscale=scale, norm_type=None, act_type='leakyrelu',
                          mode='CNA', res_scale=1, upsample_mode='upconv')
    if tiled or tiled_x8 or tiled_many or tiled_u8 or set_x8:
        try:
            # the library's own refusal, before anything is loaded
            model._x4_only('--tile-x8' if tiled_x8 else '--tile-many' if tiled_many else '--tile-u8' if tiled_u8 else
                           '--tile-many-x8' if tiles['--tile-many-x8'] else '--tile-u8-x8' if tiles['--tile-u8-x8'] else '--tile')
        except ValueError as e:
            sys.exit('sr_infer.py: %s' % e)
    sd = synth.rrdbnet_state_dict(23, 0, upscale=scale) if model_path == 'synthetic' else torch.load(model_path, map_location='cpu')
    model.load_state_dict(sd, strict=False)           # test_image/test.py:17
    model.eval()
    for _, v in model.named_parameters():
        v.requires_grad = False
    model = model.to(dev).set_precision(prec)
    os.makedirs(out_dir, exist_ok=True)
    if tiled_many:
        return run_tile_many(model, dev, in_dir, out_dir, *tiled_many)
    if tiled_u8:
        return run_tile_u8(model, dev, in_dir, out_dir, *tiled_u8)
    if tiles['--tile-many-x8']:
        return run_tile_many(model, dev, in_dir, out_dir, *tiles['--tile-many-x8'], x8=True)
    if tiles['--tile-u8-x8']:
        return run_tile_u8(model, dev, in_dir, out_dir, *tiles['--tile-u8-x8'], x8=True)
    for idx, path in enumerate(sorted(glob.glob(os.path.join(in_dir, '*'))), 1):
        base = os.path.splitext(os.path.basename(path))[0]
        img = np.array(Image.open(path).convert('RGB')).astype(np.float64) / 255
        x = torch.from_numpy(np.transpose(img, (2, 0, 1))).float().unsqueeze(0).to(dev)
        with torch.no_grad():
            y = (model.forward_tiled_x8(x, *tiled_x8) if tiled_x8 else model.forward_tiled(x, *tiled) if tiled else
                 model.forward_x8(x) if x8 else model(x))
            out = y.data.squeeze().float().cpu().clamp_(0, 1).numpy()
        out = (np.transpose(out, (1, 2, 0)) * 255.0).round().astype(np.uint8)
        Image.fromarray(out).save(os.path.join(out_dir, '%s_rlt.png' % base))
        print(idx, base, img.shape[:2], '->', out.shape[:2])


def run_tile_many(model, dev, in_dir, out_dir, tile, pad=16, x8=False):
    """--tile-many: the folder through ``forward_tiled_many`` in flushes of at least 4 x 16 windows; the same per-image
    arithmetic, files and lines as the loop of ``main``.  x8: through ``forward_tiled_many_x8``."""
    queue, windows = [], 0

    def flush():
        with torch.no_grad():
            ys = (model.forward_tiled_many_x8 if x8 else model.forward_tiled_many)([x for _, _, _, x in queue], tile, pad)
            outs = [y.data.squeeze().float().cpu().clamp_(0, 1).numpy() for y in ys]
        for (idx, base, shape, _), out in zip(queue, outs):
            out = (np.transpose(out, (1, 2, 0)) * 255.0).round().astype(np.uint8)
            Image.fromarray(out).save(os.path.join(out_dir, '%s_rlt.png' % base))
            print(idx, base, shape, '->', out.shape[:2])
        del queue[:]

    for idx, path in enumerate(sorted(glob.glob(os.path.join(in_dir, '*'))), 1):
        base = os.path.splitext(os.path.basename(path))[0]
        img = np.array(Image.open(path).convert('RGB')).astype(np.float64) / 255
        queue.append((idx, base, img.shape[:2], torch.from_numpy(np.transpose(img, (2, 0, 1))).float().unsqueeze(0).to(dev)))
        windows += -(-img.shape[0] // max(tile, 1)) * -(-img.shape[1] // max(tile, 1))
        if windows >= 4 * 16:
            flush()
            windows = 0
    if queue:
        flush()


def run_tile_u8(model, dev, in_dir, out_dir, tile, pad=16, x8=False):
    """--tile-u8: run_tile_many's flushes through ``forward_images``; uint8 HWC up, uint8 HWC down, the same files and
    lines.  x8: ``forward_images(x8=True)``."""
    queue, windows = [], 0

    def flush():
        with torch.no_grad():
            outs = [y.cpu().numpy() for y in model.forward_images([x for _, _, x in queue], tile, pad, x8=x8)]
        for (idx, base, x), out in zip(queue, outs):
            Image.fromarray(out).save(os.path.join(out_dir, '%s_rlt.png' % base))
            print(idx, base, tuple(x.shape[:2]), '->', out.shape[:2])
        del queue[:]

    for idx, path in enumerate(sorted(glob.glob(os.path.join(in_dir, '*'))), 1):
        base = os.path.splitext(os.path.basename(path))[0]
        x = torch.from_numpy(np.array(Image.open(path).convert('RGB'))).to(dev)
        queue.append((idx, base, x))
        windows += -(-x.shape[0] // max(tile, 1)) * -(-x.shape[1] // max(tile, 1))
        if windows >= 4 * 16:
            flush()
            windows = 0
    if queue:
        flush()


if __name__ == '__main__':
    main()
