"""When the kernel-side weight copies are rebuilt, re-packed and re-gathered: the change-detection contract of
WeightPack / DgradPack and the dense-block weight streams that are gathered from them.  Weights only, no images."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def small_convs(dev, seed=0):
    """Six small convs; index 1 is outside the storages that either pack samples on its fast path."""
    g = torch.Generator().manual_seed(seed)
    shapes = [(32, 64, 3, True), (32, 64, 3, True), (3, 32, 3, True),      # 32 -> 3: bias through the padded arena
              (64, 64, 1, False), (32, 32, 3, True), (32, 32, 3, True)]
    out = []
    for i, (co, ci, ks, bias) in enumerate(shapes):
        w = torch.nn.Parameter((torch.randn(co, ci, ks, ks, generator=g) * 0.1).to(dev))
        b = torch.nn.Parameter(torch.randn(co, generator=g).to(dev)) if bias else None
        out.append(('c%d' % i, w, b))
    return out


def make_pack(kind, convs, prec, dev):
    from esrganplus_amd import engine as E
    if kind == 'weight':
        return E.WeightPack(convs, prec, dev)
    return E.DgradPack([(k, w) for k, w, _ in convs], prec, dev, {})


def packed_bytes(pack):
    torch.cuda.synchronize()
    out = [pack.arena.cpu()]
    if hasattr(pack, 'bias_arena'):
        out.append(pack.bias_arena.cpu())
    return out


def same_as_fresh(pack, kind, convs, prec, dev, st):
    fresh = make_pack(kind, convs, prec, dev)
    fresh.ensure(st, force=False)
    a, b = packed_bytes(pack), packed_bytes(fresh)
    return all(torch.equal(x, y) for x, y in zip(a, b)) and bool(a[0].any())


@pytest.mark.parametrize('prec', ['fp16', 'fp32'])
@pytest.mark.parametrize('kind', ['weight', 'dgrad'])
def test_repack_state_machine(dev, kind, prec):
    """(generation, pack_count) after every step: storage changes rebuild the op list (generation), every run of the
    pack launch counts once (pack_count), and nothing else moves either."""
    from esrganplus_amd import engine as E
    st = E.current_stream()
    convs = small_convs(dev)
    pack = make_pack(kind, convs, prec, dev)
    state = lambda: (pack.generation, pack.pack_count)
    pack.ensure(st, force=False)
    assert state() == (1, 1)                                   # the first call builds and packs
    assert same_as_fresh(pack, kind, convs, prec, dev, st)
    pack.ensure(st, force=False)
    assert state() == (1, 1)                                   # nothing changed: nothing packed
    with torch.no_grad():
        convs[2][1].add_(1.0)                                  # _version bumps
        convs[2][2].add_(1.0)
    pack.ensure(st, force=False)
    assert state() == (1, 2)
    assert same_as_fresh(pack, kind, convs, prec, dev, st)
    pack.ensure(st, force=True)                                # forced: packs, leaves no signature ...
    assert state() == (1, 3)
    pack.ensure(st, force=False)                               # ... so the next non-forced call packs again
    assert state() == (1, 4)
    pack.ensure(st, force=True, record_sig=True)               # forced with a recorded signature ...
    assert state() == (1, 5)
    pack.ensure(st, force=False)                               # ... the next non-forced call relies on it
    assert state() == (1, 5)
    g = torch.Generator().manual_seed(7)
    p = convs[1][1]
    held = [p.data]                                            # (the stale op list still reads the old storages)
    if kind == 'weight':
        p.data = (torch.randn(p.shape, generator=g) * 0.1).to(dev).clone()    # no _version bump, not a sampled storage
        pack.ensure(st, force=False)
        assert state() == (1, 5)                               # (8th call) not seen by the sampled fingerprint
        pack.ensure(st, force=False, full=True)
        assert state() == (2, 6)                               # full=True: rebuilt at once, and packed
        assert same_as_fresh(pack, kind, convs, prec, dev, st)
        held.append(p.data)
    p.data = (torch.randn(p.shape, generator=g) * 0.1).to(dev).clone()
    gen, count = state()
    for n in range(1, pack.FULL_CHECK_EVERY + 1):              # found by the periodic full comparison at the latest
        pack.ensure(st, force=True)
        assert pack.pack_count == count + n
        if pack.generation != gen:
            break
    assert pack.generation == gen + 1
    assert same_as_fresh(pack, kind, convs, prec, dev, st)


@pytest.mark.parametrize('prec,direction', [('fp16', 'fwd'), ('fp32', 'fwd'), ('fp16', 'bwd')])
def test_streams_are_the_table_gather_of_the_pack(dev, prec, direction):
    """The stream arena is the pack's arena gathered with the table, byte for byte; the forward bias vector is the five
    biases of a block end to end; the gather runs again exactly when the pack ran."""
    from esrganplus_amd import block as B, engine as E
    st = E.current_stream()
    torch.manual_seed(3)
    rrdb = B.RRDB(64).to(dev).set_precision(prec)
    prefixes = ['rrdb.RDB1', 'rrdb.RDB2']
    if direction == 'fwd':
        pack = E.WeightPack(rrdb._conv_list(), prec, dev)
        streams = E.RdbStreams(pack, prefixes)
    else:
        pack = rrdb._new_dgrad_pack(dev)
        streams = E.RdbBwdStreams(pack, prefixes)

    def gathered():
        torch.cuda.synchronize()
        src = pack.arena.cpu().numpy().reshape(-1, 1024)
        tab = np.asarray(streams._table(), dtype=np.int64)
        assert not (tab % 1024).any() and tab.min() >= 0 and tab.max() < src.shape[0] * 1024
        return src[tab // 1024].reshape(-1)
    pack.ensure(st, force=False)
    streams.ensure(st)
    want = gathered()
    assert want.any() and np.array_equal(streams.arena.cpu().numpy(), want)
    if direction == 'fwd':
        bias = torch.cat([getattr(getattr(rrdb, 'RDB%d' % j), 'conv%d' % k)[0].bias.detach()
                          for j in (1, 2) for k in range(1, 6)])
        assert bias.numel() == 2 * 192 and torch.equal(streams.bias.cpu(), bias.cpu())
    streams.arena.fill_(0xFF)
    pack.ensure(st, force=False)                               # the pack did not run ...
    streams.ensure(st)
    torch.cuda.synchronize()
    assert bool((streams.arena == 0xFF).all())                 # ... so nothing was gathered
    with torch.no_grad():
        rrdb.RDB2.conv3[0].weight.mul_(0.5)
    pack.ensure(st, force=False)                               # it ran: gathered again, from the new weights
    streams.ensure(st)
    again = gathered()
    assert not np.array_equal(again, want) and np.array_equal(streams.arena.cpu().numpy(), again)
