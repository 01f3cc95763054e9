"""The instantiations chain_launch (csrc/rdb_fused.hip) chooses between for one fp16 chain: regular geometry vs general,
traced vs trace-free (csrc/rdb_chain_kernel.h: REG, TRC).  All of them must store the same bits.

Inference cases: ONE RRDB = a chain of 3 dense blocks (tests/chain_stage_refs.block_module('rrdb'), eval, fp16) driven
through engine.Builder the way Builder.block_plan does, at
  (1, 64, 32, 64)   2 x 2 sixteen-row tiles: every tile has side and corner neighbours          -> regular
  (80, 64, 32, 64)  320 tiles on 256 CUs: workgroups take a second ticket                        -> regular
  (1, 64, 24, 40)   a ragged bottom row of tiles and a ragged right column                       -> general
The float64 reference is chain_stage_refs.emulate_blocks (every stored stage rounded to fp16, as the chain stores it).
Bound: the fp16 bound of tests/test_gpu_chain_stages.py, 1.5e-3 of the reference's largest magnitude, for the chain's
output.  Each test prints its figure before it asserts.  At B = 80 the images are image 0 rolled along H and W (zero
padding makes each a case of its own): images 0, 37, 64 and 79 have a reference — 64 and 79 lie in tiles 256..319, the
ones a workgroup takes with its second ticket.

Training case: RRDBNet nb = 1 forward + backward at 16 x 3 x 32 x 32 (the 4-row builds), trace-free vs traced."""
import pytest
import torch

from tests import chain_stage_refs as R

pytestmark = pytest.mark.gpu

TOL = 1.5e-3            # TOL['fp16'] of tests/test_gpu_chain_stages.py
REF_IMAGES = (0, 37, 64, 79)
POISON = 0x5A5A5A5A5A5A5A5A


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
def knobs(monkeypatch):
    from esrganplus_amd import _lib as L
    monkeypatch.setenv('ESR_RDB_ROWS', '4')            # 16-row tiles whatever the tile count
    yield
    L.lib().esr_debug_chain_force_general(-1)


class Chain:
    """The RRDB as one mode-0 chain launch over (B, 64, H, W)"""

    def __init__(self, mod, B, H, W, dev):
        from esrganplus_amd import engine as E
        self.E, self.dev, self.shape = E, dev, (B, 64, H, W)
        bld = E.Builder(mod._weights(dev), B, H, W, 'fp16', dev, False, mod.variant, 'rrdb', 1)
        assert E.rdb_chain_ok(B, H, W, False, False)
        P = self.P = bld.plan
        xa, xb = bld.buf(64), bld.buf(64)
        P.in_op = bld.import_nchw(xa, 64)
        self.k = bld.rdb_chain(bld.rrdb_chain_specs('rrdb', 0, xa, xb))
        P.out_op = bld.export_nchw(xa, 64)
        P.out_shape = self.shape
        ch = P.ops.ops[self.k].u.rdb_chain
        assert ch.n_blocks == 3 and ch.mode == 0
        self.bld = bld

    def run(self, x, general=False, trace=None):
        from esrganplus_amd import _lib as L
        lib = L.lib()
        lib.esr_debug_chain_force_general(1 if general else 0)
        self.P.ops.ops[self.k].u.rdb_chain.trace = trace.data_ptr() if trace is not None else None
        self.P.ops._arr = None
        out = torch.empty(self.shape, dtype=torch.float32, device=self.dev)
        self.P.run(x, out, self.E.current_stream())
        torch.cuda.synchronize()
        variant = lib.esr_debug_chain_last_variant()
        assert int(self.P.chain_ws[1].item()) == 0, 'a bounded spin of the chain timed out'
        assert lib.esr_rdb_check_abort() == 0
        return out.cpu(), variant


_REF = {}


def reference(sd, x):
    key = tuple(x.shape)
    if key not in _REF:
        xs, _ = R.emulate_blocks(sd, R.block_prefixes('rrdb'), x, tails={2: 0}, prec='fp16')
        _REF[key] = xs[-1]
    return _REF[key]


def test_regular_and_general_chains_store_the_same_bits(dev, rrdb):
    from esrganplus_amd import _lib as L
    mod, sd = rrdb
    x1 = R.randn((1, 64, 32, 64), 151)
    ref = reference(sd, x1)
    c1 = Chain(mod, 1, 32, 64, dev)
    reg, v = c1.run(x1.to(dev))
    assert v & L.CHAIN_VARIANT_REGULAR and not v & L.CHAIN_VARIANT_TRACED and v >> 8 == 4, v
    gen, v = c1.run(x1.to(dev), general=True)
    assert not v & L.CHAIN_VARIANT_REGULAR and v >> 8 == 4, v
    e_reg, e_gen = R.rel_err(reg, ref), R.rel_err(gen, ref)
    print('B = 1: err / scale regular %.3e general %.3e (bound %.1e)' % (e_reg, e_gen, TOL))
    assert torch.equal(reg, gen)
    assert e_reg <= TOL and e_gen <= TOL
    # 320 tiles: the images are the one above rolled along H and W; every image is held to the regular = general
    # identity, REF_IMAGES to their own references as well
    # (shifts 7 b mod 31 and 11 b mod 63: zero only for image 0, which stays the B = 1 input)
    x80 = torch.stack([torch.roll(x1[0], (7 * b % 31, 11 * b % 63), (1, 2)) for b in range(80)])
    c80 = Chain(mod, 80, 32, 64, dev)
    reg80, v = c80.run(x80.to(dev))
    assert v & L.CHAIN_VARIANT_REGULAR, v
    gen80, v = c80.run(x80.to(dev), general=True)
    assert not v & L.CHAIN_VARIANT_REGULAR, v
    assert torch.equal(reg80, gen80)
    assert torch.equal(reg80[:1], reg)                   # a tile's result does not depend on the ticket it came with
    for b in REF_IMAGES:
        rb = ref if b == 0 else R.emulate_blocks(sd, R.block_prefixes('rrdb'), x80[b:b + 1], tails={2: 0}, prec='fp16')[0][-1]
        e_reg, e_gen = R.rel_err(reg80[b:b + 1], rb), R.rel_err(gen80[b:b + 1], rb)
        print('B = 80, image %d: err / scale regular %.3e general %.3e (bound %.1e)' % (b, e_reg, e_gen, TOL))
        assert e_reg <= TOL and e_gen <= TOL, b


def test_a_ragged_shape_takes_the_general_chain(dev, rrdb):
    from esrganplus_amd import _lib as L
    mod, sd = rrdb
    x = R.randn((1, 64, 24, 40), 152)
    out, v = Chain(mod, 1, 24, 40, dev).run(x.to(dev))
    assert not v & L.CHAIN_VARIANT_REGULAR and not v & L.CHAIN_VARIANT_TRACED and v >> 8 == 4, v
    e = R.rel_err(out, reference(sd, x))
    print('24 x 40: err / scale %.3e (bound %.1e)' % (e, TOL))
    assert e <= TOL


def test_a_traced_launch_stores_the_same_bits_and_an_untraced_one_leaves_the_trace_alone(dev, rrdb):
    from esrganplus_amd import _lib as L
    mod, _ = rrdb
    x = R.randn((1, 64, 32, 64), 151).to(dev)
    c = Chain(mod, 1, 32, 64, dev)
    ntiles = 4
    tr = torch.full((ntiles * 64,), POISON, dtype=torch.int64, device=dev)
    plain, v = c.run(x)
    assert not v & L.CHAIN_VARIANT_TRACED
    assert (tr.cpu() == POISON).all()
    tr.zero_()
    traced, v = c.run(x, trace=tr)
    assert v & L.CHAIN_VARIANT_TRACED and not v & L.CHAIN_VARIANT_REGULAR, v
    assert torch.equal(plain, traced)
    t = tr.cpu().view(ntiles, 64)
    n = int((t[0] != 0).sum())
    assert n >= 20, 'stamps of the second block: %d' % n           # tools/chain_trace.py names 28 of them
    for tile in range(ntiles):
        s = t[tile, :n]
        assert (s > 0).all() and (s[1:] >= s[:-1]).all(), (tile, s.tolist())
        assert (t[tile, n:] == 0).all()
    # .. and a launch without the pointer leaves a poisoned buffer as it is
    tr.fill_(POISON)
    again, v = c.run(x)
    assert not v & L.CHAIN_VARIANT_TRACED and torch.equal(again, plain)
    assert (tr.cpu() == POISON).all()


def test_training_chains_traced_and_trace_free_store_the_same_bits(dev, monkeypatch):
    """RRDBNet nb = 1 (3 dense blocks), forward + backward at 16 x 32^2 LR: output, input gradient and every parameter
    gradient of a step whose two chains carry trace stamps equal those of the trace-free step bit for bit."""
    from esrganplus_amd import architecture as arch, synth, _lib as L
    monkeypatch.delenv('ESR_RDB_ROWS', raising=False)
    monkeypatch.setenv('ESR_RDB_TRAIN_CHAIN', '1')
    net = arch.RRDBNet(3, 3, 64, 1).to(dev).train(False).set_precision('fp16')
    net.load_state_dict(synth.rrdbnet_state_dict(nb=1, seed=5), strict=True)
    x0 = synth.image_batch(153, 16, 3, 32, 32, name='variants.x').to(dev)
    gy = R.randn((16, 3, 128, 128), 154).to(dev)

    def step():
        x = x0.clone().requires_grad_(True)
        net.zero_grad(set_to_none=True)
        y = net(x)
        y.backward(gy)
        torch.cuda.synchronize()
        v = L.lib().esr_debug_chain_last_variant()
        return [y.detach().cpu(), x.grad.cpu()] + [p.grad.cpu() for p in net.parameters() if p.grad is not None], v

    plain, v = step()
    assert not v & L.CHAIN_VARIANT_TRACED
    tp = [p for p in net._plans.values() if isinstance(p, list)][0][0]
    assert tp.fwd.chain_ops and tp.bwd_chain_ops, 'the fused training chains were not chosen'
    tr = torch.zeros(2, 256 * 64, dtype=torch.int64, device=dev)
    tp.fwd.ops.array()[tp.fwd.chain_ops[0]].u.rdb_chain.trace = tr[0].data_ptr()
    tp.bwd.array()[tp.bwd_chain_ops[0]].u.rdb_chain.trace = tr[1].data_ptr()
    traced, v = step()
    assert v & L.CHAIN_VARIANT_TRACED, v
    assert (tr[0] != 0).any() and (tr[1] != 0).any(), 'the traced chains left no stamps'
    assert len(plain) == len(traced)
    for n, (a, b) in enumerate(zip(plain, traced)):
        assert torch.equal(a, b), 'tensor %d differs' % n
    assert L.lib().esr_rdb_check_abort() == 0
