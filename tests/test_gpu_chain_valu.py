"""The fp16 dense-block chains after the VALU diet of their epilogues and block tail (csrc/rdb_chain_kernel.h: the
pair-typed value flow from accumulator to packed row, store addressing hoisted out of the row loop, `+ x2` and the
carry into the next block's conv5 accumulators through v_fma_mix_f32, the carry read back from the LDS behind publish).
Every build that shares the header runs once, at the smallest shape that selects it, against float64:

  a  (1, 64, 48, 96)   one RRDB = 3 dense blocks on 3 x 3 sixteen-row tiles: the centre tile has all eight neighbours,
                       blocks 2 and 3 start from a carried 5 x, block 3 has the RRDB tail.  Regular chain, and the general
                       chain (esr_debug_chain_force_general, the in-process ESR_RDB_GENERAL=1) bit for bit
  b  (1, 64, 24, 40)   ragged bottom and right tiles: the general chain; the carry of a pixel beyond the image is 0
  c  (1, 64, 16, 32), (1, 64, 8, 32), (33, 64, 32, 32)   the short-tile builds as the dispatch picks them
                       (rows_per_wave, csrc/rdb_fused.hip: the smallest tile whose launch is one round of workgroups):
                       BOTH small shapes take the 4-row tiles (rdb_rows1: 4 and 2 tiles), a shape takes the 8-row tiles
                       (rdb_rows2) only when its 4-row tiles outnumber the CUs — 33 x 8 = 264 > 256 is the smallest
                       batch of 32 x 32 that does.  Its images are image 0 rolled; images 0 and 32 have a reference
  d  (2, 64, 32, 32)   training forward + backward of an RRDB, noise off (block_module 'rrdb', eval) and on ('rrdb_ti',
                       train), stage by stage as tests/test_gpu_chain_stages.py checks them, with the tile height the
                       library picks (4 rows) and with 16-row tiles
  e  (1, 64, 4097, 1)  257 tiles of 16 x 32 for 256 CUs: the smallest image that cannot be one launch and runs in row
                       bands (rdb_fused_band; engine.rdb_band_geometry: 2 bands of 2064 rows), driven through
                       Builder.rdb_chain_banded with a layout op in place of the head conv

Inference reference: chain_stage_refs.emulate_blocks (float64, every stored stage rounded to fp16); measure and bound
those of tests/test_gpu_chain_variants.py: largest error relative to the reference's largest magnitude <= 1.5e-3.
Training: chain_stage_refs stage references through test_gpu_chain_stages.check_train_plan (same bound per stage).
Each test prints its figures before it asserts."""
import pytest
import torch

from tests import chain_stage_refs as R
from tests import test_gpu_chain_stages as ST
from tests.test_gpu_chain_variants import Chain, TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def rrdb(dev):
    mod = R.block_module('rrdb').to(dev).eval().set_precision('fp16')
    sd = {k: v.detach().cpu() for k, v in mod.state_dict().items()}
    return mod, sd


@pytest.fixture(autouse=True)
def knobs():
    from esrganplus_amd import _lib as L
    yield
    L.lib().esr_debug_chain_force_general(-1)


def rrdb_reference(sd, x, prefixes=None):
    return R.emulate_blocks(sd, prefixes or R.block_prefixes('rrdb'), x, tails={2: 0}, prec='fp16')[0][-1]


def test_a_nine_regular_tiles_regular_and_general_bit_for_bit(dev, rrdb, monkeypatch):
    from esrganplus_amd import _lib as L
    monkeypatch.setenv('ESR_RDB_ROWS', '4')
    mod, sd = rrdb
    x = R.randn((1, 64, 48, 96), 161)
    c = Chain(mod, 1, 48, 96, dev)
    reg, v = c.run(x.to(dev))
    assert v & L.CHAIN_VARIANT_REGULAR and not v & L.CHAIN_VARIANT_TRACED and v >> 8 == 4, v
    gen, v = c.run(x.to(dev), general=True)
    assert not v & L.CHAIN_VARIANT_REGULAR and v >> 8 == 4, v
    ref = rrdb_reference(sd, x)
    e_reg, e_gen = R.rel_err(reg, ref), R.rel_err(gen, ref)
    print('48 x 96: err / scale regular %.3e general %.3e (bound %.1e)' % (e_reg, e_gen, TOL))
    assert torch.equal(reg, gen)
    assert e_reg <= TOL and e_gen <= TOL


def test_b_a_ragged_shape_on_the_general_chain(dev, rrdb, monkeypatch):
    from esrganplus_amd import _lib as L
    monkeypatch.setenv('ESR_RDB_ROWS', '4')
    mod, sd = rrdb
    x = R.randn((1, 64, 24, 40), 162)
    out, v = Chain(mod, 1, 24, 40, dev).run(x.to(dev))
    assert not v & L.CHAIN_VARIANT_REGULAR and not v & L.CHAIN_VARIANT_TRACED and v >> 8 == 4, v
    e = R.rel_err(out, rrdb_reference(sd, x))
    print('24 x 40: err / scale %.3e (bound %.1e)' % (e, TOL))
    assert e <= TOL


@pytest.mark.parametrize('shape,rows,ref_images', [((1, 64, 16, 32), 1, (0,)), ((1, 64, 8, 32), 1, (0,)), ((33, 64, 32, 32), 2, (0, 32))],
                         ids=['1x16x32-rows1', '1x8x32-rows1', '33x32x32-rows2'])
def test_c_the_short_tile_builds_as_the_dispatch_picks_them(dev, rrdb, monkeypatch, shape, rows, ref_images):
    from esrganplus_amd import _lib as L
    monkeypatch.delenv('ESR_RDB_ROWS', raising=False)
    assert L.lib().esr_rdb_max_tiles_per_image() == 256, 'the shapes of this case are chosen for 256 CUs'
    mod, sd = rrdb
    B, _, H, W = shape
    x0 = R.randn((1, 64, H, W), 163)
    x = torch.stack([torch.roll(x0[0], (5 * b % 31, 3 * b % 29), (1, 2)) for b in range(B)])
    out, v = Chain(mod, B, H, W, dev).run(x.to(dev))
    assert not v & L.CHAIN_VARIANT_REGULAR and not v & L.CHAIN_VARIANT_TRACED and v >> 8 == rows, v
    for b in ref_images:
        e = R.rel_err(out[b:b + 1], rrdb_reference(sd, x[b:b + 1]))
        print('%s image %d (%d rows per wave): err / scale %.3e (bound %.1e)' % (shape, b, rows, e, TOL))
        assert e <= TOL, b


@pytest.mark.parametrize('kind,train,rows', [('rrdb', False, None), ('rrdb_ti', True, None), ('rrdb', False, '4'), ('rrdb_ti', True, '4')],
                         ids=['noise-off-auto', 'noise-on-auto', 'noise-off-rows4', 'noise-on-rows4'])
def test_d_training_forward_and_backward_stage_by_stage(dev, monkeypatch, kind, train, rows):
    monkeypatch.setenv('ESR_RDB_TRAIN_CHAIN', '1')
    if rows is None:
        monkeypatch.delenv('ESR_RDB_ROWS', raising=False)
    else:
        monkeypatch.setenv('ESR_RDB_ROWS', rows)
    shape = (2, 64, 32, 32)
    mod = R.block_module(kind).to(dev).train(train).set_precision('fp16')
    sd = {k: v.detach().cpu() for k, v in mod.state_dict().items()}
    bld = ST.build(mod, 'rrdb', 64, 64, 2, 32, 32, dev, train)
    seed = ST.step(bld, R.randn(shape, 164).to(dev), R.randn(shape, 165).to(dev), train)
    pre = R.block_prefixes(kind)
    ST.check_train_plan('valu case d %s rows %s' % (kind, rows or 'auto'), bld, sd, lambda i, j: pre[j], train, seed, dev)


def test_e_the_smallest_banded_launch(dev, monkeypatch):
    from esrganplus_amd import architecture as arch, engine as E, synth, _lib as L
    monkeypatch.delenv('ESR_RDB_ROWS', raising=False)
    H, W = 4097, 1
    assert L.lib().esr_rdb_max_tiles_per_image() == 256
    assert not E.rdb_chain_ok(1, H, W, False, False) and E.rdb_chain_ok(1, H - 1, W, False, False)
    geom = E.rdb_band_geometry(H, W)
    assert geom is not None and geom[2] == 2, geom
    sd = synth.rrdbnet_state_dict(nb=1, seed=21)
    net = arch.RRDBNet(3, 3, 64, 1).to(dev).eval().set_precision('fp16')
    net.load_state_dict(sd, strict=True)
    bld = E.Builder(net._weights(dev), 1, H, W, 'fp16', dev, False, net.variant, 'net', 1)
    P = bld.plan

    def layout(view, to_g32):
        lo = L.esr_layout()
        lo.dtype, lo.to_g32 = bld.dt_e, to_g32
        lo.B, lo.C, lo.H, lo.W = 1, 64, H, W
        lo.g32 = view
        return P.ops.add(L.OP_LAYOUT, 'layout', lo)

    def head(dst):
        P.in_op = layout(dst, 1)
    res = bld.rdb_chain_banded(geom, head)
    P.out_op = layout(res, 0)
    P.out_shape = (1, 64, H, W)
    assert len(P.chain_ops) == 1 and P.ops.ops[P.chain_ops[0]].u.rdb_chain.band_rows == geom[0]
    x = R.randn((1, 64, H, W), 166)
    out = torch.empty(P.out_shape, dtype=torch.float32, device=dev)
    P.run(x.to(dev), out, E.current_stream())
    torch.cuda.synchronize()
    assert int(P.chain_ws[1].item()) == 0, 'a bounded spin of the chain timed out'
    assert L.lib().esr_rdb_check_abort() == 0
    ref = rrdb_reference({k: v.detach().cpu() for k, v in sd.items()}, x, ['model.1.sub.0.RDB%d' % j for j in (1, 2, 3)])
    e = R.rel_err(out.cpu(), ref)
    print('4097 x 1 in 2 bands: err / scale %.3e (bound %.1e)' % (e, TOL))
    assert e <= TOL
