"""CPU tests of the dense-block weight streams' gather tables: which 1 KB fragment of the per-conv packed arena goes
where in the fused stream that the chain kernels consume (include/esrgan_hip.h: esr_rdb_block.w, "Backward weight
stream").  Packs and streams are built on the CPU and never run: only the offset tables are looked at."""
import hashlib

import numpy as np
import pytest

PREFIXES = ['model.1.sub.0.RDB1', 'model.1.sub.0.RDB2']
FWD = ['.conv%d.0' % k for k in range(1, 6)]             # cout blocks 0..3 and 4/5 of the forward stream
BWD = ['.g4', '.g3', '.c2', '.g1', '.c0']                # ... of the backward stream
TABLES = [('fp16', 'fwd'), ('fp32', 'fwd'), ('fp16', 'bwd')]

# sha256 over the int64 bytes of each table, offsets relative to the source arena
PINNED = {
    ('fp16', 'fwd'): 'cb01e7958a5b25a60194dc394353f419ce8508fa35c7f66d6adefd3d6b029376',
    ('fp32', 'fwd'): '39d1e24d45554ad557226532640f77265e430cc6f63b97a04b286dfe532f6f89',
    ('fp16', 'bwd'): '1d1d74506773b06c672631c40014a2f17f782f7e1badb62f330f3ba9771c2fda',
}


@pytest.fixture(scope='module')
def tables():
    """(precision, direction) -> (pack, streams, table as int64 array); the nets are kept alive with it."""
    import __graft_entry__ as ge
    ge.build()
    from esrganplus_amd import architecture as arch, engine as E
    out, keep = {}, []
    for prec in ('fp16', 'fp32'):
        net = arch.RRDBNet(3, 3, 64, 1).set_precision(prec)
        keep.append(net)
        wp = E.WeightPack(net._conv_list(), prec, 'cpu', net._subpix_keys())
        todo = [('fwd', wp, E.RdbStreams(wp, PREFIXES))]
        if prec == 'fp16':
            dp = net._new_dgrad_pack('cpu')
            todo.append(('bwd', dp, E.RdbBwdStreams(dp, PREFIXES)))
        for direction, pack, streams in todo:
            out[prec, direction] = (pack, streams, np.asarray(streams._table(), dtype=np.int64))
    out['keep'] = keep
    return out


@pytest.mark.parametrize('which', TABLES, ids='-'.join)
def test_stream_table_is_the_recorded_one(tables, which):
    """The table is the one commit 0af93ec ("Split the conv-net plan builder into a SeqBuilder with named steps")
    built.  The literals in PINNED were produced there, with the `tables` fixture of this file unchanged, by
        for k in TABLES:
            print(k, hashlib.sha256(tables[k][2].tobytes()).hexdigest())
    and are never regenerated from later code: a change of the unit order is a change of the kernel's contract."""
    assert hashlib.sha256(tables[which][2].tobytes()).hexdigest() == PINNED[which]


@pytest.mark.parametrize('which', TABLES, ids='-'.join)
def test_stream_table_gathers_every_fragment_of_its_block_exactly_once(tables, which):
    from esrganplus_amd import _lib as L
    pack, streams, tab = tables[which]
    sfx, one = (FWD, '.conv1x1') if which[1] == 'fwd' else (BWD, '.o1')
    n = streams.stream_bytes // 1024
    assert streams.stream_bytes % 1024 == 0 and len(tab) == len(PREFIXES) * n
    base, seen = pack.arena.data_ptr(), set()
    for i, p in enumerate(PREFIXES):
        got = tab[i * n:(i + 1) * n].tolist()
        want = set()
        for s in sfx + [one]:
            e = pack.entries[p + s]
            nbytes = L.packed_weight_bytes(e.cout, e.cin, e.ks, pack.esr_dtype)
            assert nbytes % 1024 == 0
            want |= set(range(e.w_ptr - base, e.w_ptr - base + nbytes, 1024))
        assert all(o % 1024 == 0 for o in got)
        assert len(set(got)) == n and set(got) == want      # a bijection onto this block's fragments, no other block's
        assert not (seen & want)
        seen |= want


@pytest.mark.parametrize('which', TABLES, ids='-'.join)
def test_the_1x1_sits_where_the_header_says(tables, which):
    """Unit counts of include/esrgan_hip.h (esr_rdb_block.w), c = K steps of the phase's input slice (64 / cpg for
    x, 32 / cpg for x1..x4): crit_p = c * 3 kw * 3 kh fragments of conv_p alone, bulk_p = c * 3 kw * (6 - p) cout
    blocks * 3 kh.  fp16 forward: behind bulk_1; fp16 backward: behind crit_3; fp32: at the end of the stream."""
    pack, streams, tab = tables[which]
    kx, kd = 64 // pack.cpg, 32 // pack.cpg
    crit = lambda p: (kx if p == 1 else kd) * 9
    bulk = lambda p: (kx if p == 1 else kd) * 3 * (6 - p) * 3
    n = streams.stream_bytes // 1024
    e1 = pack.entries[PREFIXES[1] + ('.conv1x1' if which[1] == 'fwd' else '.o1')]
    n_one = kx if which[1] == 'fwd' else 4
    if which == ('fp16', 'fwd'):
        at = crit(1) + bulk(1)
    elif which == ('fp16', 'bwd'):
        at = crit(1) + bulk(1) + crit(2) + bulk(2) + crit(3)
    else:
        at = n - n_one
    one = [e1.w_ptr - pack.arena.data_ptr() + 1024 * f for f in range(n_one)]
    assert tab[n + at:n + at + n_one].tolist() == one        # (looked at in the SECOND block: per-block bases count)
