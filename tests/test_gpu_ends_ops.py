"""The two ends of every inference form of RRDBNet, at the smallest shapes at which each can still go wrong (nb = 1): the
result against the form's pure-torch reference (bit identity), the cached plan's op list — the form's input op, the ops
of the ordinary plan of the same batch shape, the form's output op, with HR_conv1 in front of it where the output goes
through the plan's fp32 slots buffer — and the per-run fields of the two end ops after the call, which hold the last
pass's values.  Then ``StreamOrder``: a call that raises still records its end."""
import pytest
import torch

from esrganplus_amd import functional as F
from esrganplus_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _net(dev, prec='fp16'):
    from esrganplus_amd import architecture as arch
    net = arch.RRDBNet(3, 3, 64, 1).to(dev).eval()
    net.load_state_dict(synth.rrdbnet_state_dict(nb=1, seed=81), strict=True)
    net.max_cached_plans = 32          # the form's plans and the ordinary plans of its reference stay cached side by side
    return net.set_precision(prec)


def _same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _plans_of(cached):
    """The engine Plans behind an entry of ``net._plans``: ``.plans`` on the x8 kinds, ``.plan`` on the tiled kinds, the
    entry itself for ``net(x)``."""
    if hasattr(cached, 'plans'):
        return list(cached.plans)
    return [getattr(cached, 'plan', cached)]


def _sig(arr, i0, i1):
    """Ops [i0, i1) of an op array by kind, the convs with (ks, upsample, H, W, B)."""
    from esrganplus_amd import _lib as L
    out = []
    for i in range(i0, i1):
        c = arr[i].u.conv
        out.append((arr[i].kind, c.ks, c.upsample, c.H, c.W, c.B) if arr[i].kind == L.OP_CONV else (arr[i].kind,))
    return out


def _check_ends(net, plan, kind, union, want_in, want_out, dev):
    """The op list of `plan` is [kind] + the ordinary plan's ops behind its import + [kind] (kind OP_LAYOUT, the plain
    ends: the ordinary plan's own list, HR_conv1 is the output op), and the fields of the two end ops hold want_in /
    want_out."""
    from esrganplus_amd import _lib as L
    arr, n = plan.ops.array(), len(plan.ops.ops)
    plain = kind == L.OP_LAYOUT
    assert plan.in_op == 0 and arr[0].kind == kind and plan.out_op == n - 1
    assert arr[n - 1].kind == (L.OP_CONV if plain else kind) and arr[n - 2].kind == L.OP_CONV
    g, s = (arr[0].u.layout, arr[n - 1].u.conv) if plain else (getattr(arr[0].u, union), getattr(arr[n - 1].u, union))
    for op, want in ((g, want_in), (s, want_out)):                # (first: the plain ends' plan IS the ordinary plan)
        for name, v in want.items():
            assert getattr(op, name) == v, (name, getattr(op, name), v)
    if not plain:
        hr1 = arr[n - 2].u.conv.nchw_out
        assert g.to_g32 == 1 and s.to_g32 == 0
        assert hr1 and s.slots_nchw == hr1                        # HR_conv1 writes the buffer the output op reads
    fea = arr[1].u.conv
    B, H, W = fea.B, fea.H, fea.W
    with torch.no_grad():
        net(torch.zeros(B, 3, H, W, device=dev))
    ordinary = net._plans[(B, H, W, net.precision, False, False, net._weights(dev).generation)]
    oarr, on = ordinary.ops.array(), len(ordinary.ops.ops)
    assert oarr[0].kind == L.OP_LAYOUT and ordinary.in_op == 0
    assert oarr[on - 1].kind == L.OP_CONV and ordinary.out_op == on - 1
    assert _sig(arr, 1, n if plain else n - 1) == _sig(oarr, 1, on)       # the middle and HR_conv1


def _only_entry(net, kind=None):
    keys = [k for k in net._plans if kind is None or k[0] == kind]
    assert len(keys) == 1 and len(net._plans) == 1, list(net._plans)
    return net._plans[keys[0]]


def test_forward_plain_ends(dev):
    from esrganplus_amd import _lib as L
    from oracle import ref_torch as RT
    net = _net(dev)
    x = synth.image_batch(3, 1, 3, 8, 12, name='ends.fwd').to(dev)
    with torch.no_grad():
        y = net(x)
        (plan,) = _plans_of(_only_entry(net))
        y2 = net(x)
        assert _same_bits(y2, y) and _plans_of(_only_entry(net)) == [plan]
        ref = RT.rrdbnet_forward(x.cpu(), synth.rrdbnet_state_dict(nb=1, seed=81), 1)
    assert tuple(y.shape) == (1, 3, 32, 48) and plan.out_shape == (1, 3, 32, 48)
    assert (y.cpu() - ref).abs().max().item() <= 5e-2             # the project's fp16 gate against the fp32 oracle
    _check_ends(net, plan, L.OP_LAYOUT, 'layout', dict(nchw=x.data_ptr(), B=1, C=3, H=8, W=12, to_g32=1),
                dict(nchw_out=y2.data_ptr(), nchw_out_c=3), dev)


def _chunked(net, n):
    """The net's forward in batches of n: what a pass of n slots x images runs."""
    return lambda xb: torch.cat([net(c.contiguous()) for c in xb.split(n, 0)], 0)


@pytest.mark.parametrize('shape,slots_arg,slots,last', [
    ((1, 3, 8, 8), None, 8, [(0, 0, 0.125)]),                                  # one plan, one pass
    ((2, 3, 8, 12), 2, 2, [(2, 1, 1.0), (6, 1, 0.125)]),                        # two plans, four chained passes
])
def test_forward_x8_ends(dev, monkeypatch, shape, slots_arg, slots, last):
    from esrganplus_amd import _lib as L
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    net = _net(dev)
    B, _, H, W = shape
    x = synth.image_batch(4, *shape, name='ends.x8').to(dev)
    with torch.no_grad():
        y = net.forward_x8(x) if slots_arg is None else net.forward_x8(x, slots_per_pass=slots_arg)
        entry = _only_entry(net, 'x8')
        plans = _plans_of(entry)
        ref = F.x8_reference(_chunked(net, slots * B), x)
    assert _same_bits(y, ref)
    assert entry.slots == slots and tuple(entry.out_shape) == (B, 3, 4 * H, 4 * W)
    assert len(plans) == len(last)
    for plan, (k0, acc, scale), (ph, pw) in zip(plans, last, [(H, W), (W, H)]):
        fea = plan.ops.array()[1].u.conv
        assert (fea.B, fea.H, fea.W) == (slots * B, ph, pw)
        assert tuple(plan.out_shape) == (B, 3, 4 * H, 4 * W)
        _check_ends(net, plan, L.OP_DIHEDRAL, 'dihedral',
                    dict(nchw=x.data_ptr(), B=B, C=3, H=H, W=W, k_begin=k0, k_count=slots, accumulate=0, scale=1.0),
                    dict(nchw=y.data_ptr(), B=B, C=3, H=4 * H, W=4 * W, k_begin=k0, k_count=slots, accumulate=acc,
                         scale=scale), dev)


@pytest.mark.parametrize('prec', ['fp16', 'fp32'])
def test_forward_tiled_ends(dev, prec):
    """2 x 3 x 20 x 27, tile 8, pad 2: 3 x 4 tiles of 12 x 12 windows, 5 per pass — the third pass holds 2 tiles and 3
    repeats of the last."""
    from esrganplus_amd import _lib as L
    net = _net(dev, prec)
    x = synth.image_batch(5, 2, 3, 20, 27, name='ends.tiled').to(dev)
    with torch.no_grad():
        y = net.forward_tiled(x, 8, 2, 5)
        entry = _only_entry(net, 'tiled')
        ref = F.tiled_reference(net, x, 8, 2, 5)
    assert _same_bits(y, ref)
    assert [k[:5] for k in net._plans if k[0] == 'tiled'] == [('tiled', 5, 2, 12, 12)]
    (plan,) = _plans_of(entry)
    fea = plan.ops.array()[1].u.conv
    assert (fea.B, fea.H, fea.W) == (10, 12, 12) and tuple(plan.out_shape) == (10, 3, 48, 48)
    _check_ends(net, plan, L.OP_TILE, 'tile',
                dict(nchw=x.data_ptr(), B=2, C=3, H=20, W=27, tile=8, pad=2, scale=1, t_begin=10, t_count=5),
                dict(nchw=y.data_ptr(), B=2, C=3, H=80, W=108, tile=8, pad=2, scale=4, t_begin=10, t_count=5), dev)


def test_forward_tiled_x8_ends(dev, monkeypatch):
    """1 x 3 x 10 x 27, tile 8, pad 2: 2 x 4 tiles of 10 x 12 windows, so two plans (10 x 12 for k 0..3, 12 x 10 for k
    4..7); 2 tiles and 2 slots per pass: four tile passes of four k passes each."""
    from esrganplus_amd import _lib as L
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    net = _net(dev)
    x = synth.image_batch(6, 1, 3, 10, 27, name='ends.tiled_x8').to(dev)
    with torch.no_grad():
        y = net.forward_tiled_x8(x, 8, 2, tiles_per_pass=2, slots_per_pass=2)
        entry = _only_entry(net, 'tiled_x8')
        ref = F.tiled_x8_reference(net, x, 8, 2, 2, 2)
    assert _same_bits(y, ref)
    assert [k[:6] for k in net._plans if k[0] == 'tiled_x8'] == [('tiled_x8', 2, 2, 1, 10, 12)]
    plans = _plans_of(entry)
    assert len(plans) == 2 and entry.slots == 2
    for plan, (k0, scale), (ph, pw) in zip(plans, [(2, 1.0), (6, 0.125)], [(10, 12), (12, 10)]):
        fea = plan.ops.array()[1].u.conv
        assert (fea.B, fea.H, fea.W) == (4, ph, pw)
        common = dict(B=1, C=3, tile=8, pad=2, t_begin=6, t_count=2, k_begin=k0, k_count=2)
        _check_ends(net, plan, L.OP_TILE_X8, 'tile_x8',
                    dict(common, nchw=x.data_ptr(), H=10, W=27, scale=1, accumulate=0, mean_scale=1.0),
                    dict(common, nchw=y.data_ptr(), H=40, W=108, scale=4, accumulate=1, mean_scale=scale), dev)


SIZES = [(9, 20), (20, 9), (13, 13)]      # tile 8, pad 2: 6, 6 and 4 windows of 9 x 12, 12 x 9 and 12 x 12
GROUPS = [(5, 9, 12), (5, 12, 9), (4, 12, 12)]      # (slots, th, tw) at 5 windows per pass: filler in the first two


def _check_set_plans(net, kind, op_kind, union, dev, **extra):
    keys = [k for k in net._plans if k[0] == kind]
    assert [k[:4] for k in keys] == [(kind,) + g for g in GROUPS] and len(net._plans) == 3, list(net._plans)
    plans = [net._plans[k] for k in keys]
    for entry, (S, th, tw) in zip(plans, GROUPS):
        (plan,) = _plans_of(entry)
        fea = plan.ops.array()[1].u.conv
        assert (fea.B, fea.H, fea.W) == (S, th, tw) and tuple(plan.out_shape) == (S, 3, 4 * th, 4 * tw)
        common = dict(C=3, tile=8, pad=2, th=th, tw=tw, n_slots=S, **extra)
        _check_ends(net, plan, op_kind, union, dict(common, scale=1), dict(common, scale=4), dev)
    return plans


def test_forward_tiled_many_ends(dev):
    from esrganplus_amd import _lib as L
    net = _net(dev)
    xs = [synth.image_batch(7 + i, 1, 3, H, W, name='ends.many').to(dev)[0] for i, (H, W) in enumerate(SIZES)]
    with torch.no_grad():
        ys = net.forward_tiled_many(xs, 8, 2, 5)
        plans = _check_set_plans(net, 'tiled_many', L.OP_TILE_MANY, 'tile_many', dev)
        refs = F.tiled_many_reference(net, xs, 8, 2, 5)
    assert len(ys) == 3 and all(_same_bits(y, r) for y, r in zip(ys, refs))
    assert [tuple(y.shape) for y in ys] == [(3, 4 * H, 4 * W) for H, W in SIZES]
    for p in plans:                      # the item pointers of the last pass lie in one table: gather entries, then stitch
        (plan,) = _plans_of(p)
        arr = plan.ops.array()
        assert 0 < arr[plan.in_op].u.tile_many.items < arr[plan.out_op].u.tile_many.items


def test_forward_images_ends_one_plan_for_both_channel_orders(dev):
    from esrganplus_amd import _lib as L
    net = _net(dev)
    g = torch.Generator().manual_seed(11)
    xs = [torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev) for H, W in SIZES]
    with torch.no_grad():
        rgb = net.forward_images(xs, 8, 2, 5)
        plans = _check_set_plans(net, 'tiled_img', L.OP_TILE_IMG, 'tile_img', dev, bgr=0)
        cached = {k: v for k, v in net._plans.items() if k[0] == 'tiled_img'}
        bgr = net.forward_images(xs, 8, 2, 5, bgr=True)
        assert {k: v for k, v in net._plans.items() if k[0] == 'tiled_img'} == cached
        for k in [k for k in net._plans if k[0] != 'tiled_img']:
            del net._plans[k]            # (the ordinary plans _check_set_plans built for its comparison)
        assert _check_set_plans(net, 'tiled_img', L.OP_TILE_IMG, 'tile_img', dev, bgr=1) == plans
        ref_rgb = F.images_reference(net, xs, 8, 2, 5)
        ref_bgr = F.images_reference(net, xs, 8, 2, 5, bgr=True)
    for ys, refs in ((rgb, ref_rgb), (bgr, ref_bgr)):
        assert len(ys) == 3 and all(_same_bits(y, r) for y, r in zip(ys, refs))
        assert all(y.dtype == torch.uint8 and tuple(y.shape) == (4 * H, 4 * W, 3) for y, (H, W) in zip(ys, SIZES))
    assert not all(_same_bits(a, b) for a, b in zip(rgb, bgr))


def test_a_raising_call_still_records_its_end(dev, monkeypatch):
    """Plan.run raises before any launch (a Python exception only) in a call from a side stream: the module's stream
    order names that stream afterwards, and the next call from the default stream is an ordinary one."""
    from esrganplus_amd import engine as E
    net = _net(dev)
    x = synth.image_batch(3, 1, 3, 8, 12, name='ends.order').to(dev)
    side = torch.cuda.Stream(device=dev)

    def refuse(self, *a, **kw):
        raise RuntimeError('refused before any launch')
    with torch.no_grad():
        want = _net(dev)(x)
        torch.cuda.synchronize()
        with monkeypatch.context() as m:
            m.setattr(E.Plan, 'run', refuse)
            with torch.cuda.stream(side), pytest.raises(RuntimeError, match='refused before any launch'):
                net(x)
        assert E.StreamOrder.of(net).last == side.cuda_stream
        assert _same_bits(net(x), want)
