"""Glue between the drop-in nn.Modules and the recorded HIP launch plans."""
import os

import torch

from . import engine as E
from . import _lib as L


def _draw_seed():
    """Philox key of one training forward: torch's CPU generator (reproducible under torch.manual_seed,
    utils/util.py:43-47) mixed with the data-parallel rank — every rank seeds torch identically
    (set_random_seed), and identical keys would inject the SAME GaussianNoise field into the ranks' different
    local batches instead of independent noise over the global batch."""
    s = int(torch.randint(0, 2 ** 62, (1,)).item())
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        s = (s ^ (torch.distributed.get_rank() * 0x9E3779B97F4A7C15)) & (2 ** 62 - 1)
    return s


def _needs_grad(module, x):
    if not torch.is_grad_enabled():
        return False
    # (a nn.DataParallel replica holds its weights as plain attributes — `parameters()` is empty there — so ask the
    # attribute-access list the launches use)
    ps = module._convs()[1] if hasattr(module, '_convs') else list(module.parameters())
    return x.requires_grad or any(p.requires_grad for p in ps)


def _prep_input(x, what):
    E.require_cuda(x, what)
    if x.dim() != 4:
        raise ValueError('%s must be NCHW, got shape %s' % (what, tuple(x.shape)))
    if x.shape[2] == 0 or x.shape[3] == 0:
        # torch's Conv2d rejects these too ("Kernel size can't be greater than actual input size")
        raise ValueError('%s has an empty spatial extent: shape %s' % (what, tuple(x.shape)))
    return x.detach().contiguous().float()


def _zs_list(z, n, shape, device):
    if z is None:
        return None
    zs = list(z) if isinstance(z, (list, tuple)) else [z]
    if len(zs) != n:
        raise ValueError('expected %d noise tensors, got %d' % (n, len(zs)))
    out = []
    for t in zs:
        E.require_cuda(t, 'noise tensor z')
        if tuple(t.shape) != tuple(shape):
            raise ValueError('noise tensor shape %s != %s' % (tuple(t.shape), tuple(shape)))
        out.append(t.detach().contiguous().float())
    return out


def run_block(mod, kind, x, z=None):
    """ResidualDenseBlock_5C / RRDB forward (block.py:260-268, 287-291) on the HIP path."""
    if x.dim() == 4 and x.shape[0] == 0:
        E.require_cuda(x, 'input')
        return x.new_zeros(tuple(x.shape), dtype=torch.float32)
    if _needs_grad(mod, x):
        E.require_cuda(x, 'input')
        B, C_, H, W = x.shape
        if C_ != 64:
            raise ValueError('expected 64 input channels, got %d' % C_)
        has_noise = getattr(mod, 'noise', None) is not None if kind == 'rdb' else True
        noise = bool(mod.training and has_noise)
        n_noise = E.NoiseLayers(mod.variant, kind, 1, noise).total
        zs = _zs_list(z, n_noise, (B, 64, H, W), x.device) if noise else None
        return _BlockFn.apply(x, mod, kind, noise, zs, *mod._convs()[1])
    xin = _prep_input(x, 'input')
    B, C_, H, W = xin.shape
    if C_ != 64:
        raise ValueError('expected 64 input channels, got %d' % C_)
    with E.StreamOrder.of(mod).call():
        wp = mod._weights(xin.device)
        has_noise = getattr(mod, 'noise', None) is not None if kind == 'rdb' else True
        noise = bool(mod.training and has_noise)
        n_noise = E.NoiseLayers(mod.variant, kind, 1, noise).total
        zs = _zs_list(z, n_noise, (B, 64, H, W), xin.device) if noise else None
        key = (kind, B, H, W, mod.precision, noise, zs is not None, wp.generation)
        plan = mod._plans.get(key)
        if plan is None:
            plan = E.build_block_plan(kind, wp, B, H, W, mod.precision, xin.device, noise,
                                      mod.variant, zs is not None)
            mod._plans = {key: plan}
        out = torch.empty(plan.out_shape, dtype=torch.float32, device=xin.device)
        plan.run(xin, out, E.current_stream(), _draw_seed() if (noise and zs is None) else 0, zs)
    return out


def _train_forward(tp, xin, st, seed, zs):
    if tp.graph:
        tp.x_static.copy_(xin)
        tp.seed_t.fill_(seed)
        if tp.fwd.streams is not None:          # the chain's weight streams are gathered outside the graph
            tp.fwd.streams.ensure(st)
        tp.fwd.ops.graph_launch(st)
        return tp.out_static.clone()
    out = torch.empty(tp.fwd.out_shape, dtype=torch.float32, device=xin.device)
    tp.fwd.run(xin, out, st, seed, zs)
    return out


def _train_backward(tp, gy, st, noise, explicit, seed, want_gx, sync=None, prepared=False, follow_wgs=None):
    """Runs the backward launch list; returns dL/dx (stand-alone blocks) or None.
    follow_wgs: workgroups of the follower pass of weight gradients for THIS run (None: the plan's default); the
    results do not depend on it.
    prepared: the gradient buffers are zeroed and the backward chain's weight streams gathered already
    (`rrdbnet_train_prepare`, on another stream the caller has ordered in front of this one)."""
    if not prepared:
        tp.grad_flat.zero_()
        if tp.tapmajor is not None:
            tp.tapmajor.tm.zero_()
        for t in tp.scratch_grads:
            t.zero_()
    if tp.graph:
        tp.gy_static.copy_(gy)
        if tp.bwd_streams is not None:
            tp.bwd_streams.ensure(st)
        tp.bwd.graph_launch(st)                 # seed_t still holds this step's seed
        return tp.gx_static.clone() if (want_gx and tp.gx_op is not None) else None
    arr = tp.bwd.array()
    arr[tp.gy_op].u.layout.nchw = gy.data_ptr()
    gx = None
    n_ops = len(tp.bwd.ops)
    if tp.gx_begin is not None and not want_gx:
        n_ops = tp.gx_begin                         # whole generator: fea_conv's input gradient only on request
    elif tp.gx_op is not None:
        gx = torch.empty(tp.gx_shape, dtype=torch.float32, device=gy.device)
        E.set_nchw(arr[tp.gx_op], gx.data_ptr())
    mode = L.NOISE_OFF
    if noise:
        mode = L.NOISE_EXPLICIT if explicit else L.NOISE_PHILOX
    for i in tp.bwd_noise_ops:
        arr[i].u.conv.noise_mode = mode
        arr[i].u.conv.seed = seed
    if tp.follow_op is not None:
        arr[tp.follow_op].u.rdb_wgrad.max_workgroups = (max(32, min(int(follow_wgs), tp.follow_spare)) if follow_wgs
                                                        else tp.follow_wgs)
    for i in tp.bwd_chain_ops:                      # fused backward chain (esr_rdb_backward): same Philox key as the forward
        arr[i].u.rdb_chain.noise_mode = L.NOISE_PHILOX if noise else L.NOISE_OFF
        arr[i].u.rdb_chain.seed = seed
    if tp.bwd_streams is not None and not prepared:
        tp.bwd_streams.ensure(st)
    if tp.segments is None or sync is None:
        tp.bwd.run_range(st, 0, n_ops)
        return gx
    # data-parallel: hand every finished slice of the flat gradient buffer to `sync` (an asynchronous
    # all-reduce, dp.GradExchange) as soon as the ops that produce it are enqueued — slices are merged up to
    # sync.bucket_elems so that a collective moves enough bytes per xGMI link — and wait for all of them
    # (stream-side) before the gradients leave the node
    i0, pend_lo, pend_hi, handles = 0, None, None, []
    limit = getattr(sync, 'bucket_elems', 0)
    for op_end, lo, hi in tp.segments:
        tp.bwd.run_range(st, i0, op_end)
        i0 = op_end
        if pend_lo is not None and (hi != pend_lo and lo != pend_hi):
            handles.append(sync(tp.grad_flat[pend_lo:pend_hi]))
            pend_lo = None
        pend_lo, pend_hi = (lo, hi) if pend_lo is None else (min(lo, pend_lo), max(hi, pend_hi))
        if pend_hi - pend_lo >= limit:
            handles.append(sync(tp.grad_flat[pend_lo:pend_hi]))
            pend_lo = None
    tp.bwd.run_range(st, i0, n_ops)
    if pend_lo is not None:
        handles.append(sync(tp.grad_flat[pend_lo:pend_hi]))
    if hasattr(sync, 'wait_handles'):
        sync.wait_handles(handles)                  # dp.GradExchange (optionally timed: bench.py dp_train)
    else:
        for h in handles:
            if h is not None:
                h.wait()
    return gx


def _grad_views(tp):
    """Parameter gradients as views of a fresh copy of the plan's flat gradient buffer (the plan's own
    buffer is overwritten by the next backward).  One split + one view per tensor: building ~770
    slices by hand cost 3 ms of host time per step."""
    meta = tp.__dict__.get('_grad_meta')
    if meta is None:
        sizes, shapes = [], []
        for gw, gb in tp.grad_views:
            sizes.append(gw.numel())
            shapes.append(gw.shape)
            if gb is not None:
                sizes.append(gb.numel())
                shapes.append(gb.shape)
        meta = tp._grad_meta = (sizes, shapes)
    flat = tp.grad_flat.clone()
    return [t.view(sh) for t, sh in zip(flat.split(meta[0]), meta[1])]


MAX_TRAIN_SHAPES = 4    # shapes whose training plans (saved activations) a module keeps


class _PlanLease:
    """Marks a TrainPlan busy while an autograd graph still references its saved activations."""

    def __init__(self, tp):
        self.tp = tp
        tp.busy = True

    def release(self):
        if self.tp is not None:
            self.tp.busy = False
            self.tp = None

    def __del__(self):
        self.release()


def _train_plan(net, wp, dp, B, H, W, dev, noise, explicit):
    sync = getattr(net, '_grad_sync', None)      # dp.GradExchange attached: segmented backward, no graph replay
    key = ('train', B, H, W, net.precision, noise, explicit, wp.generation, str(dev), sync is not None)
    pool = net._plans.get(key)
    if pool is None:
        # every shape keeps a full set of saved activations alive: bound the number of shapes (LRU over the
        # train keys; a pool with a plan still referenced by a live autograd graph is never dropped)
        tkeys = [k for k in net._plans if isinstance(k, tuple) and k and k[0] == 'train']
        while len(tkeys) >= MAX_TRAIN_SHAPES:
            victim = next((k for k in tkeys if not any(tp.busy for tp in net._plans[k])), None)
            if victim is None:
                break
            del net._plans[victim]
            tkeys.remove(victim)
        pool = []
    else:
        del net._plans[key]              # re-insert below: most recently used last
    net._plans[key] = pool
    for tp in pool:
        if not tp.busy:
            tp.packs = (wp, dp)
            return tp
    tp = E.build_rrdbnet_train_plan(net, wp, dp, net.nb, net.in_nc, net.out_nc, B, H, W,
                                    net.precision, dev, noise, net.variant, explicit, segmented=sync is not None,
                                    scale=net.upscale)
    if not explicit and E.use_graphs() and sync is None:
        tp.enable_graph((B, net.in_nc, H, W), dev)
    # The launch lists hold RAW pointers into the packed operands: the plan keeps the packs alive.  An autograd graph
    # references the plan (through its lease), not the module — and a nn.DataParallel replica (networks.py:105-107) is
    # gone when its forward returns: without this its input-gradient operands were freed memory by the time the backward
    # ran (found in round 5 with two replicas on one GPU: wrong gradients whenever the allocator re-used the block)
    tp.packs = (wp, dp)
    pool.append(tp)
    return tp


class _RRDBNetFn(torch.autograd.Function):
    """RRDBNet forward/backward as ONE autograd node (architecture.py:76-78 + the implicit
    autograd backward triggered at SRRaGAN_model.py:140)."""

    @staticmethod
    def forward(ctx, x, net, zs, proxy, *params):
        # proxy (a 1-element leaf that requires grad) stands for ALL parameters: their gradients then leave the node
        # through net._deliver_flat_grads instead of one autograd output each; `params` is empty in that mode
        xin = _prep_input(x, 'input')
        B, _, H, W = xin.shape
        dev = xin.device
        st = E.current_stream()
        wp = net._weights(dev)
        dp = net._dgrad_weights(dev)
        dp.ensure(st, force=not net._dgrad_fresh())
        noise = bool(net.training)
        tp = _train_plan(net, wp, dp, B, H, W, dev, noise, zs is not None)
        ctx.lease = _PlanLease(tp)
        ctx.seed = _draw_seed() if (noise and zs is None) else 0
        ctx.explicit = zs is not None
        ctx.noise = noise
        ctx.n_params = len(params)
        ctx.net = net if proxy is not None else None
        ctx.sync = getattr(net, '_grad_sync', None)
        return _train_forward(tp, xin, st, ctx.seed, zs)

    @staticmethod
    def backward(ctx, gy):
        tp = ctx.lease.tp
        if tp is None:
            raise RuntimeError('RRDBNet backward called twice (retain_graph is not supported: the '
                               'saved activations live in a reusable launch plan)')
        gy = gy.detach().contiguous().float()
        if ctx.net is not None:
            ctx.net._release_adopted(tp.grad_flat)      # `.grad` may alias the buffer this backward is about to rewrite
        gx = _train_backward(tp, gy, E.current_stream(), ctx.noise, ctx.explicit, ctx.seed,
                             bool(ctx.needs_input_grad[0]), ctx.sync)
        gx = gx if ctx.needs_input_grad[0] else None
        if ctx.net is not None:
            ctx.net._deliver_flat_grads(tp.grad_flat)
            ctx.lease.release()
            return (gx, None, None, None)
        grads = _grad_views(tp)
        ctx.lease.release()
        assert len(grads) == ctx.n_params
        grads = [g if need else None for g, need in zip(grads, ctx.needs_input_grad[4:])]
        return (gx, None, None, None) + tuple(grads)


class TrainPass:
    """State of one RRDBNet training forward outside autograd (train.ESRGANPlusStep's hand-written step)."""
    __slots__ = ('lease', 'seed', 'noise', 'explicit', 'sync', 'prepared', 'pack_ev')


_ADOPT = os.environ.get('ESR_ADOPT_GRADS', '1') != '0'     # A/B knob: 0 = always copy into the module's store (round 4)


def rrdbnet_train_forward(net, x, z=None):
    """RRDBNet.forward in training form (every activation the backward needs is kept) WITHOUT an autograd node:
    returns (y, state) for ``rrdbnet_train_backward``.  Same plans, same launches as ``_RRDBNetFn``."""
    xin = _prep_input(x, 'input')
    B, C_, H, W = xin.shape
    if C_ != net.in_nc:
        raise ValueError('expected %d input channels, got %d' % (net.in_nc, C_))
    dev = xin.device
    st = E.current_stream()
    noise = bool(net.training)
    zs = _zs_list(z, E.NoiseLayers(net.variant, 'net', net.nb).total, (B, 64, H, W), dev) if noise else None
    wp = net._weights(dev)
    dp = net._dgrad_weights(dev)
    n_packs = dp.pack_count
    dp.ensure(st, force=not net._dgrad_fresh())
    pack_ev = None
    if dp.pack_count != n_packs and not torch.cuda.is_current_stream_capturing():
        # the input-gradient operands were re-packed on THIS stream just now (first step, after
        # load_state_dict / resume): whoever gathers the backward chain's weight streams from dp.arena on another
        # stream (`rrdbnet_train_prepare` on the train step's side stream) has to wait for it — recorded here, in
        # front of the forward's launches, so that the wait does not cover the forward
        pack_ev = torch.cuda.Event()
        pack_ev.record(torch.cuda.current_stream())
    tp = _train_plan(net, wp, dp, B, H, W, dev, noise, zs is not None)
    s = TrainPass()
    s.pack_ev = pack_ev
    s.lease = _PlanLease(tp)
    s.seed = _draw_seed() if (noise and zs is None) else 0
    s.noise, s.explicit, s.sync = noise, zs is not None, getattr(net, '_grad_sync', None)
    s.prepared = False
    return _train_forward(tp, xin, st, s.seed, zs), s


def rrdbnet_train_prepare(net, s):
    """What the backward of the forward state `s` needs before its first launch and that depends on nothing of this
    step — the flat gradient buffer and the tap-major arena zeroed (67 + 67 MB of fills), the backward chain's weight
    streams gathered from the input-gradient packs — enqueued on the CURRENT stream: the train step runs it on its side
    stream under the generator's forward and makes the main stream wait for it in front of the backward (three launches
    and their dispatch gaps off the step's critical path)."""
    tp = s.lease.tp
    if tp is None or tp.graph or s.prepared:
        return
    if s.pack_ev is not None:
        torch.cuda.current_stream().wait_event(s.pack_ev)     # the operands the gather below reads (see the forward)
    net._release_adopted(tp.grad_flat)
    tp.grad_flat.zero_()
    if tp.tapmajor is not None:
        tp.tapmajor.tm.zero_()
    for t in tp.scratch_grads:
        t.zero_()
    if tp.bwd_streams is not None:
        tp.bwd_streams.ensure(E.current_stream())
    s.prepared = True


def rrdbnet_train_backward(net, s, gy, follow_wgs=None):
    """The backward of ``rrdbnet_train_forward``: parameter gradients into the module's flat store (every parameter's
    ``.grad`` = its view of it, block._PlannedModule._deliver_flat_grads); dL/dx is not formed."""
    tp = s.lease.tp
    if tp is None:
        raise RuntimeError('rrdbnet_train_backward called twice on one forward')
    if not s.prepared:
        net._release_adopted(tp.grad_flat)
    _train_backward(tp, gy, E.current_stream(), s.noise, s.explicit, s.seed, False, s.sync, prepared=s.prepared,
                    follow_wgs=follow_wgs)
    net._deliver_flat_grads(tp.grad_flat, adopt=_ADOPT)
    s.lease.release()


def _block_train_plan(mod, kind, wp, dp, B, H, W, dev, noise, explicit):
    key = ('train', kind, B, H, W, mod.precision, noise, explicit, wp.generation, str(dev))
    pool = mod._plans.setdefault(key, [])
    for tp in pool:
        if not tp.busy:
            tp.packs = (wp, dp)
            return tp
    tp = E.build_rrdbnet_train_plan(mod, wp, dp, 1, 64, 64, B, H, W, mod.precision, dev, noise,
                                    mod.variant, explicit, kind=kind)
    if not explicit and E.use_graphs():
        tp.enable_graph((B, 64, H, W), dev)
    tp.packs = (wp, dp)              # (the lists hold raw pointers into the packs: see _train_plan)
    pool.append(tp)
    return tp


class _BlockFn(torch.autograd.Function):
    """Stand-alone ResidualDenseBlock_5C / RRDB (block.py:260-268, 287-291) forward + backward as one
    autograd node; unlike the whole generator it also returns the gradient w.r.t. its input."""

    @staticmethod
    def forward(ctx, x, mod, kind, noise, zs, *params):
        xin = _prep_input(x, 'input')
        B, _, H, W = xin.shape
        dev = xin.device
        st = E.current_stream()
        wp = mod._weights(dev)
        dp = mod._dgrad_weights(dev)
        dp.ensure(st)
        tp = _block_train_plan(mod, kind, wp, dp, B, H, W, dev, noise, zs is not None)
        ctx.lease = _PlanLease(tp)
        ctx.seed = _draw_seed() if (noise and zs is None) else 0
        ctx.explicit, ctx.noise, ctx.n_params = zs is not None, noise, len(params)
        return _train_forward(tp, xin, st, ctx.seed, zs)

    @staticmethod
    def backward(ctx, gy):
        tp = ctx.lease.tp
        if tp is None:
            raise RuntimeError('backward called twice (retain_graph is not supported: the saved '
                               'activations live in a reusable launch plan)')
        gy = gy.detach().contiguous().float()
        # (a stand-alone block never adopts the plan's gradient buffer: autograd accumulates copies of the views)
        gx = _train_backward(tp, gy, E.current_stream(), ctx.noise, ctx.explicit, ctx.seed, True)
        grads = _grad_views(tp)
        ctx.lease.release()
        assert len(grads) == ctx.n_params
        grads = [g if need else None for g, need in zip(grads, ctx.needs_input_grad[5:])]
        return (gx if ctx.needs_input_grad[0] else None, None, None, None, None) + tuple(grads)


def _flat_grad_route(net, params):
    """True when the backward may hand the parameter gradients over as ONE flat buffer (`_deliver_flat_grads`)."""
    return bool(net.flat_param_grads) and all(p.requires_grad and p.is_leaf for p in params)


def _cached_plan(mod, key, build):
    """``mod._plans[key]``, built by ``build()`` on first use.  A full cache is emptied before the build, so that the old
    plans' buffers are free when the new one allocates its own."""
    plan = mod._plans.get(key)
    if plan is None:
        if len(mod._plans) >= mod.max_cached_plans:
            mod._plans.clear()
        plan = mod._plans[key] = build()
    return plan


def _eval_front(net, x, s):
    """The front of an eval entry of RRDBNet at upscale s -> (xin, None), the checked fp32 NCHW input, or (None, the
    result of an empty batch: torch returns an empty result)."""
    if x.dim() == 4 and x.shape[0] == 0:
        E.require_cuda(x, 'input')
        return None, x.new_zeros((0, net.out_nc, s * x.shape[2], s * x.shape[3]), dtype=torch.float32)
    xin = _prep_input(x, 'input')
    if xin.shape[1] != net.in_nc:
        raise ValueError('expected %d input channels, got %d' % (net.in_nc, xin.shape[1]))
    return xin, None


def run_rrdbnet(net, x, z=None):
    """RRDBNet.forward (architecture.py:76-78) on the HIP path."""
    if not (x.dim() == 4 and x.shape[0] == 0) and _needs_grad(net, x):
        E.require_cuda(x, 'input')
        B, C_, H, W = x.shape
        if C_ != net.in_nc:
            raise ValueError('expected %d input channels, got %d' % (net.in_nc, C_))
        zs = _zs_list(z, E.NoiseLayers(net.variant, 'net', net.nb).total, (B, 64, H, W), x.device) if net.training else None
        params = net._convs()[1]
        # the flat route assigns `.grad` itself, which only means something on LEAF parameters: under a multi-device
        # nn.DataParallel (networks.py:105-107) a replica's weights are Broadcast outputs, and their gradient has to
        # travel back through autograd to the originals -> per-tensor outputs
        if _flat_grad_route(net, params):
            proxy = net.__dict__.get('_grad_proxy')
            if proxy is None or proxy.device != x.device:
                proxy = net.__dict__['_grad_proxy'] = torch.zeros(1, device=x.device, requires_grad=True)
            return _RRDBNetFn.apply(x, net, zs, proxy)
        net._flush_stale_grads()
        return _RRDBNetFn.apply(x, net, zs, None, *params)
    xin, empty = _eval_front(net, x, net.upscale)
    if xin is None:
        return empty
    B, _, H, W = xin.shape
    dev = xin.device
    with E.StreamOrder.of(net).call():
        wp = net._weights(dev)
        noise = bool(net.training)
        zs = _zs_list(z, E.NoiseLayers(net.variant, 'net', net.nb).total, (B, 64, H, W), dev) if noise else None
        plan = _cached_plan(net, (B, H, W, net.precision, noise, zs is not None, wp.generation),
                            lambda: E.build_rrdbnet_plan(wp, net.nb, net.in_nc, net.out_nc, B, H, W, net.precision, dev,
                                                         noise, net.variant, zs is not None, scale=net.upscale))
        out = torch.empty(plan.out_shape, dtype=torch.float32, device=dev)
        plan.run(xin, out, E.current_stream(), _draw_seed() if (noise and zs is None) else 0, zs)
    return out


def x8_transform(x, k):
    """Transform k = 0..7 of the self-ensemble, the reference's list order (codes/models/SR_model.py:103-105): bit 0 flips
    along W ('v'), bit 1 along H ('h'), bit 2 transposes ('t'); v and h first, t last."""
    if k & 1:
        x = x.flip(3)
    if k & 2:
        x = x.flip(2)
    if k & 4:
        x = x.transpose(2, 3)
    return x.contiguous()


def x8_inverse(y, k):
    """Undoes transform k on an output, in the reference's order (SR_model.py:107-113): t, then h, then v."""
    if k & 4:
        y = y.transpose(2, 3)
    if k & 2:
        y = y.flip(2)
    if k & 1:
        y = y.flip(3)
    return y.contiguous()


def x8_reference(fn, x):
    """Pure-torch restatement of the reference's ``SRModel.test_x8`` (codes/models/SR_model.py:82-120) over a forward
    ``fn``: the same eight transforms in the same list order, the same inverses, and the mean per image — the reference's
    ``cat(...).mean(dim=0)`` also averages ACROSS images and is only meaningful at B = 1, where the two agree.  Square
    input runs as one call ``fn(cat of the 8 B copies)``, non-square input as two calls of 4 B (H x W, then W x H).  The
    mean is formed as seven fp32 adds in k order times 0.125 (torch's ``mean`` does not fix a summation order)."""
    B = x.shape[0]
    xs = [x8_transform(x, k) for k in range(8)]
    if x.shape[2] == x.shape[3]:
        ys = list(fn(torch.cat(xs, 0)).float().split(B, 0))
    else:
        ys = list(fn(torch.cat(xs[:4], 0)).float().split(B, 0)) + list(fn(torch.cat(xs[4:], 0)).float().split(B, 0))
    acc = x8_inverse(ys[0], 0)
    for k in range(1, 8):
        acc = acc + x8_inverse(ys[k], k)
    return acc * 0.125


def run_rrdbnet_x8(net, x, slots_per_pass=None):
    """Geometric self-ensemble of RRDBNet (the reference's ``SRModel.test_x8``, codes/models/SR_model.py:82-120) as
    batched launch plans: the eight flip / transpose copies of ``x`` are written straight into the plan's input buffer,
    run as one batch of 8 B (non-square input: 4 B at H x W, then 4 B at W x H), and the inverse transforms and the mean
    are one reduce into the result.  Noise is off whatever ``net.training`` is (the reference calls ``eval()`` first); the
    module's mode and every ``requires_grad`` are left untouched; the result [B, out_nc, sH, sW] fp32 (s = the net's
    ``upscale``) carries no gradient.  B > 1 is ensembled PER IMAGE (the reference's ``cat`` + ``mean(dim=0)`` would also average across the
    images and is only meaningful at B = 1).  slots_per_pass (8, 4, 2 or 1; default ESR_X8_SLOTS, else 8 for square and 4
    for non-square input) bounds the memory of large images: each pass runs slots x B copies.  Every pass still holds
    whole-image plans; ``run_rrdbnet_tiled_x8`` is the ensemble per window, with the memory of a tiled forward."""
    xin, empty = _eval_front(net, x, net.upscale)
    if xin is None:
        return empty
    B, _, H, W = xin.shape
    slots = E.x8_slots(H, W, slots_per_pass)
    with E.StreamOrder.of(net).call():
        wp = net._weights(xin.device)
        plan = _cached_plan(net, ('x8', slots, B, H, W, net.precision, False, False, wp.generation),
                            lambda: E.build_rrdbnet_x8_plan(wp, net.nb, net.in_nc, net.out_nc, B, H, W, net.precision,
                                                            xin.device, net.variant, slots, scale=net.upscale))
        out = torch.empty(plan.out_shape, dtype=torch.float32, device=xin.device)
        plan.run(xin, out, E.current_stream())
    return out


tiled_geometry = E.tiled_geometry


def _tiled_ints(tile, pad, per_pass, per_pass_name):
    """Validated ints (tile >= 1, pad >= 0, per_pass >= 1) of a tiled forward; per_pass_name: 'tiles_per_pass' or
    'windows_per_pass', as the caller's argument is called."""
    import operator
    vals = []
    for name, v, lo in (('tile', tile, 1), ('pad', pad, 0), (per_pass_name, per_pass, 1)):
        try:
            if isinstance(v, bool):
                raise TypeError
            v = operator.index(v)
        except TypeError:
            raise ValueError('%s of a tiled forward must be an int >= %d, got %r' % (name, lo, v))
        if v < lo:
            raise ValueError('%s of a tiled forward must be an int >= %d, got %r' % (name, lo, v))
        vals.append(v)
    return tuple(vals)


def _tiled_args(B, H, W, tile, pad, tiles_per_pass):
    """Validated (tile, pad, P) of a tiled forward: P windows per image and pass.  Values beyond the image are cut down to
    it, which changes no tile and no window."""
    tile, pad, P = _tiled_ints(tile, pad, max(1, 16 // B) if tiles_per_pass is None else tiles_per_pass, 'tiles_per_pass')
    tile, pad = min(tile, max(H, W)), min(pad, max(H, W))
    P = min(P, -(-H // tile) * -(-W // tile))
    if P * B > 65535:
        raise ValueError('tiles_per_pass x batch = %d x %d windows are more than one launch takes (65535)' % (P, B))
    return tile, pad, P


def tiled_reference(fn, x, tile, pad, tiles_per_pass=None):
    """Pure-torch restatement of the tiled forward over a x4 forward ``fn``: the geometry of include/esrgan_hip.h
    (esr_tile), the same passes of P = min(tiles_per_pass, tiles) windows per image, slot-major (window s of image b is
    batch entry s B + b), a tail pass filled up by repeating the last window — so ``fn`` always sees a batch of P B
    windows of one shape, and results are only bit-comparable between equal batch shapes — and every tile's owned
    rectangle copied out of its window's output.  Nothing is blended: the owned rectangles are disjoint."""
    B, _, H, W = x.shape
    tile, pad, P = _tiled_args(B, H, W, tile, pad, tiles_per_pass)
    th, tw, ny, nx, tiles = tiled_geometry(H, W, tile, pad)
    out = None
    for t0 in range(0, ny * nx, P):
        idx = [min(t0 + s, ny * nx - 1) for s in range(P)]
        ys = fn(torch.cat([x[:, :, tiles[t][4]:tiles[t][4] + th, tiles[t][5]:tiles[t][5] + tw] for t in idx], 0).contiguous()).float()
        if out is None:
            out = ys.new_empty((B, ys.shape[1], 4 * H, 4 * W))
        for s, t in enumerate(idx):
            if t0 + s >= ny * nx:
                break
            y0, y1, x0, x1, wy, wx = tiles[t]
            out[:, :, 4 * y0:4 * y1, 4 * x0:4 * x1] = ys[s * B:(s + 1) * B, :, 4 * (y0 - wy):4 * (y1 - wy), 4 * (x0 - wx):4 * (x1 - wx)]
    return out


def _tiled_x8_args(B, H, W, tile, pad, tiles_per_pass, slots_per_pass):
    """Validated (tile, pad, P, slots) of a tiled self-ensemble: _tiled_args' checks, the slots of E.x8_slots for the
    window shape, and P defaulting to max(1, 16 // (slots B)) windows per image and pass."""
    tile, pad, P = _tiled_args(B, H, W, tile, pad, 1 if tiles_per_pass is None else tiles_per_pass)
    slots = E.x8_slots(min(tile + 2 * pad, H), min(tile + 2 * pad, W), slots_per_pass)
    if tiles_per_pass is None:
        P = min(max(1, 16 // (slots * B)), -(-H // tile) * -(-W // tile))
    if slots * P * B > 65535:
        raise ValueError('slots x tiles_per_pass x batch = %d x %d x %d windows are more than one launch takes (65535)'
                         % (slots, P, B))
    return tile, pad, P, slots


def tiled_x8_reference(fn, x, tile, pad, tiles_per_pass=None, slots_per_pass=None):
    """Pure-torch restatement of the tiled x8 self-ensemble over a x4 forward ``fn``: ``tiled_reference``'s windows and
    passes (P windows per image, slot-major, a tail pass filled up by repeating the last window), every window — pad
    included — transformed the eight ways of ``x8_transform``, in runs of ``slots`` transforms: ``fn`` sees batches of
    slots P B windows, entry ((k - k0) P + p) B + b, th x tw for k < 4 and tw x th for k >= 4.  The outputs are
    inverse-transformed and summed as seven fp32 adds in k order, times 0.125 (``x8_reference``'s arithmetic), and every
    tile's owned rectangle of that mean is copied out.  Nothing is blended."""
    B, _, H, W = x.shape
    tile, pad, P, slots = _tiled_x8_args(B, H, W, tile, pad, tiles_per_pass, slots_per_pass)
    th, tw, ny, nx, tiles = tiled_geometry(H, W, tile, pad)
    out = None
    for t0 in range(0, ny * nx, P):
        idx = [min(t0 + s, ny * nx - 1) for s in range(P)]
        wins = torch.cat([x[:, :, tiles[t][4]:tiles[t][4] + th, tiles[t][5]:tiles[t][5] + tw] for t in idx], 0)
        acc = None
        for k0 in range(0, 8, slots):
            ys = fn(torch.cat([x8_transform(wins, k) for k in range(k0, k0 + slots)], 0)).float().split(P * B, 0)
            for k, y in zip(range(k0, k0 + slots), ys):
                acc = x8_inverse(y, k) if acc is None else acc + x8_inverse(y, k)
        mean = acc * 0.125
        if out is None:
            out = mean.new_empty((B, mean.shape[1], 4 * H, 4 * W))
        for s, t in enumerate(idx):
            if t0 + s >= ny * nx:
                break
            y0, y1, x0, x1, wy, wx = tiles[t]
            out[:, :, 4 * y0:4 * y1, 4 * x0:4 * x1] = mean[s * B:(s + 1) * B, :, 4 * (y0 - wy):4 * (y1 - wy), 4 * (x0 - wx):4 * (x1 - wx)]
    return out


def run_rrdbnet_tiled_x8(net, x, tile=96, pad=16, tiles_per_pass=None, slots_per_pass=None):
    """Tiled x8 self-ensemble of RRDBNet: the windows of ``run_rrdbnet_tiled`` (same geometry), each — pad included —
    transformed the eight ways of ``run_rrdbnet_x8``, forwarded, inverse-transformed, summed in k order and times 0.125;
    the owned rectangle of that mean is copied into the result (include/esrgan_hip.h: esr_tile_x8; nothing is blended).
    Per window, not per image: with pad >= 15 nb + 4 this is mathematically ``forward_x8(x)``, smaller pads approximate
    it.  One pass runs slots x P x B windows as one batch of the ordinary inference plan — slots from ``slots_per_pass``
    (8, 4, 2 or 1; default ESR_X8_SLOTS, else 8 for square windows and 4 otherwise: a pass cannot mix th x tw and tw x th
    slots), P = min(tiles_per_pass, tiles) — and passes of fewer than 8 slots are chained into the result.  Square
    windows need one launch plan for all eight transforms, non-square ones two; images of any size that share a window
    shape share them, and the activation memory is that of slots P B windows whatever the image — where ``forward_x8``
    holds 8 B (or 2 x 4 B) copies of the whole image.  Noise is off whatever ``net.training`` is; the module's mode and
    every ``requires_grad`` are left untouched; the result [B, out_nc, 4H, 4W] fp32 carries no gradient; B > 1 is
    ensembled per image.  The default pass — tiles_per_pass = max(1, 16 // (slots B)) windows of 128 x 128 — is the
    16 x 128 x 128 batch that bench.py measures; other pass sizes are unmeasured (profiles/tiled_x8.md)."""
    xin, empty = _eval_front(net, x, 4)
    if xin is None:
        return empty
    B, _, H, W = xin.shape
    tile, pad, P, slots = _tiled_x8_args(B, H, W, tile, pad, tiles_per_pass, slots_per_pass)
    th, tw = min(tile + 2 * pad, H), min(tile + 2 * pad, W)
    with E.StreamOrder.of(net).call():
        wp = net._weights(xin.device)
        # no H, W in the key: every image with this window shares the plan
        plan = _cached_plan(net, ('tiled_x8', slots, P, B, th, tw, net.precision, wp.generation),
                            lambda: E.build_rrdbnet_tiled_x8_plan(wp, net.nb, net.in_nc, net.out_nc, B, th, tw,
                                                                  net.precision, xin.device, net.variant, P, slots))
        out = torch.empty((B, net.out_nc, 4 * H, 4 * W), dtype=torch.float32, device=xin.device)
        plan.run(xin, out, tile, pad, E.current_stream())
    return out


def run_rrdbnet_tiled(net, x, tile=96, pad=16, tiles_per_pass=None):
    """Tiled eval forward of RRDBNet: the image is cut into windows of min(tile + 2 pad, H) x min(tile + 2 pad, W) LR
    pixels that lie inside it (shifted inward at the borders, never zero-filled), P = min(tiles_per_pass, tiles) windows
    per image run as one batch of the ordinary inference plan, and every tile's owned tile x tile rectangle is copied
    from its window's output into the result (include/esrgan_hip.h: esr_tile; nothing is blended).  Images of any size
    that share a window shape share one launch plan and its buffers, and the activation memory is that of P B windows
    whatever the image.  With pad >= 15 nb + 4 the result is mathematically the whole-image forward; smaller pads, the
    default among them for nb = 23, approximate it (profiles/tiled_inference.md).  Noise is off whatever
    ``net.training`` is; the module's mode and every ``requires_grad`` are left untouched; the result
    [B, out_nc, 4H, 4W] fp32 carries no gradient.  The defaults — 128 x 128 windows, max(1, 16 // B) of them per pass
    — are the 16 x 128 x 128 batch that bench.py measures; that choice has not been measured against other pass sizes.
    A pass costs what that batch costs, so an image the whole-image forward can take is faster through ``net(x)``
    (339 x 510: 2 passes, 17.3 against 8.5 ms in fp16): tiling bounds memory and shares the plan, it is not a speed-up.
    The x8 self-ensemble over the same windows is ``run_rrdbnet_tiled_x8``."""
    xin, empty = _eval_front(net, x, 4)
    if xin is None:
        return empty
    B, _, H, W = xin.shape
    tile, pad, P = _tiled_args(B, H, W, tile, pad, tiles_per_pass)
    th, tw = min(tile + 2 * pad, H), min(tile + 2 * pad, W)
    with E.StreamOrder.of(net).call():
        wp = net._weights(xin.device)
        # no H, W in the key: every image with this window shares the plan
        plan = _cached_plan(net, ('tiled', P, B, th, tw, net.precision, wp.generation),
                            lambda: E.build_rrdbnet_tiled_plan(wp, net.nb, net.in_nc, net.out_nc, B, th, tw, net.precision,
                                                               xin.device, net.variant, P))
        out = torch.empty((B, net.out_nc, 4 * H, 4 * W), dtype=torch.float32, device=xin.device)
        plan.run(xin, out, tile, pad, E.current_stream())
    return out


def _tiled_many_ints(tile, pad, windows_per_pass):
    """Validated ints (tile, pad, windows_per_pass) of a tiled forward over an image set."""
    return _tiled_ints(tile, pad, windows_per_pass, 'windows_per_pass')


def _tiled_many_groups(sizes, tile, pad, windows_per_pass):
    """[(th, tw, S, [(image, tiles of that image)])] per window shape, in order of first appearance: the counts behind
    ``tiled_many_passes`` without the window lists.  tile, pad, windows_per_pass are validated ints."""
    groups = {}
    for i, (H, W) in enumerate(sizes):
        if H < 1 or W < 1:
            raise ValueError('image %d of a tiled forward has no pixels: %d x %d' % (i, H, W))
        key = (min(tile + 2 * pad, H), min(tile + 2 * pad, W))
        groups.setdefault(key, []).append((i, -(-H // tile) * -(-W // tile)))
    out = []
    for (th, tw), members in groups.items():
        S = min(windows_per_pass, sum(n for _, n in members))
        if S > 65535:
            raise ValueError('windows_per_pass = %d slots of %d x %d windows are more than one launch takes (65535)' % (S, th, tw))
        out.append((th, tw, S, members))
    return out


def tiled_many_passes(sizes, tile, pad, windows_per_pass):
    """The passes of a tiled forward over images of the LR sizes ``sizes`` [(H, W)]: host code only.  Windows are grouped
    by window shape (min(tile + 2 pad, H), min(tile + 2 pad, W)) — a pass is one batch of one shape — the groups in order
    of first appearance, inside a group the images in list order and each image's tiles row-major (``tiled_geometry``).
    A group of n windows runs in ceil(n / S) passes of S = min(windows_per_pass, n) slots; only its last pass may hold
    filler, which repeats the group's last window with live = 0 (gathered, so that no slot holds stale data, never
    stitched).  -> [(th, tw, S, passes)] per group, passes a list of S-tuples (image, tile, live)."""
    tile, pad, wpp = _tiled_many_ints(tile, pad, windows_per_pass)
    out = []
    for th, tw, S, members in _tiled_many_groups([(int(h), int(w)) for h, w in sizes], tile, pad, wpp):
        wins = [(i, t, 1) for i, n in members for t in range(n)]
        passes = []
        for k in range(0, len(wins), S):
            p = wins[k:k + S]
            passes.append(tuple(p + [(wins[-1][0], wins[-1][1], 0)] * (S - len(p))))
        out.append((th, tw, S, passes))
    return out


def _tiled_many_images(images, in_nc):
    """The images of a tiled forward over an image set as a list of ([1, C, H, W] view, rank of the input): rank 3 or
    4 with one image each, in_nc channels (None: whatever the first has), at least one pixel."""
    out = []
    for i, x in enumerate(images):
        if not isinstance(x, torch.Tensor) or x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[0] != 1):
            raise ValueError('image %d of a tiled forward must be a [C, H, W] or [1, C, H, W] tensor, got %s'
                             % (i, tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__))
        v = x if x.dim() == 4 else x.unsqueeze(0)
        if in_nc is None:
            in_nc = v.shape[1]
        if v.shape[1] != in_nc:
            raise ValueError('image %d: expected %d input channels, got %d' % (i, in_nc, v.shape[1]))
        if v.shape[2] < 1 or v.shape[3] < 1:
            raise ValueError('image %d of a tiled forward has no pixels: shape %s' % (i, tuple(x.shape)))
        out.append((v, x.dim()))
    return out


def tiled_many_reference(fn, images, tile, pad, windows_per_pass=16):
    """Pure-torch restatement of the tiled forward over an image set and a x4 forward ``fn``: the passes of
    ``tiled_many_passes``, ``fn`` called on exactly those batches — S windows of one shape, filler included — and the
    owned rectangle of every live window copied out of its output into its image's result.  Nothing is blended.
    -> a list of fp32 results, [C', 4H, 4W] or [1, C', 4H, 4W] as the inputs' ranks."""
    tile, pad, wpp = _tiled_many_ints(tile, pad, windows_per_pass)
    xs = _tiled_many_images(list(images), None)
    geo = [tiled_geometry(v.shape[2], v.shape[3], tile, pad) for v, _ in xs]
    outs = [None] * len(xs)
    for th, tw, S, passes in tiled_many_passes([(v.shape[2], v.shape[3]) for v, _ in xs], tile, pad, wpp):
        for p in passes:
            wins = [xs[i][0][:, :, geo[i][4][t][4]:geo[i][4][t][4] + th, geo[i][4][t][5]:geo[i][4][t][5] + tw] for i, t, _ in p]
            ys = fn(torch.cat(wins, 0).contiguous()).float()
            for s, (i, t, live) in enumerate(p):
                if not live:
                    continue
                if outs[i] is None:
                    outs[i] = ys.new_empty((1, ys.shape[1], 4 * xs[i][0].shape[2], 4 * xs[i][0].shape[3]))
                y0, y1, x0, x1, wy, wx = geo[i][4][t]
                outs[i][:, :, 4 * y0:4 * y1, 4 * x0:4 * x1] = ys[s:s + 1, :, 4 * (y0 - wy):4 * (y1 - wy), 4 * (x0 - wx):4 * (x1 - wx)]
    return [o if rank == 4 else o[0] for o, (_, rank) in zip(outs, xs)]


def _x8_slots_arg(slots_per_pass, x8=True):
    """slots_per_pass of an image-set entry, checked before anything else is: one of E.X8_SLOTS or None, and only with
    the self-ensemble."""
    if slots_per_pass is None:
        return None
    if not x8:
        raise ValueError('slots_per_pass = %r belongs to the x8 self-ensemble: pass x8=True' % (slots_per_pass,))
    if isinstance(slots_per_pass, bool) or slots_per_pass not in E.X8_SLOTS:
        raise ValueError('slots per pass of the x8 self-ensemble must be one of %s, got %r' % (E.X8_SLOTS, slots_per_pass))
    return int(slots_per_pass)


def tiled_many_x8_passes(sizes, tile, pad, windows_per_pass=16, slots_per_pass=None):
    """The passes of the x8 self-ensemble over images of the LR sizes ``sizes`` [(H, W)]: host code only.  Groups, their
    order and the order of the windows inside a group are ``tiled_many_passes``'.  ``windows_per_pass`` counts batch
    entries of the launch plan, and a window takes ``slots = E.x8_slots(th, tw, slots_per_pass)`` of them at a time
    (8, 4, 2 or 1; 8 for square windows and 4 otherwise by default), so a pass holds
    P = min(max(1, windows_per_pass // slots), windows of the group) windows and runs 8 / slots times, once per k range
    (``E.x8_passes``); the default pass is the 16 x 128 x 128 batch that bench.py measures.  Only a group's last pass may
    hold filler, which repeats the group's last window with live = 0 (gathered for every k, never reduced).
    -> [(th, tw, slots, P, passes)] per group, passes a list of P-tuples (image, tile, live)."""
    slots_per_pass = _x8_slots_arg(slots_per_pass)
    tile, pad, wpp = _tiled_many_ints(tile, pad, windows_per_pass)
    out = []
    for th, tw, _, members in _tiled_many_groups([(int(h), int(w)) for h, w in sizes], tile, pad, 1):
        slots = E.x8_slots(th, tw, slots_per_pass)
        wins = [(i, t, 1) for i, n in members for t in range(n)]
        P = min(max(1, wpp // slots), len(wins))
        if slots * P > 65535:
            raise ValueError('slots x windows = %d x %d batch entries of %d x %d windows are more than one launch takes '
                             '(65535)' % (slots, P, th, tw))
        passes = []
        for k in range(0, len(wins), P):
            p = wins[k:k + P]
            passes.append(tuple(p + [(wins[-1][0], wins[-1][1], 0)] * (P - len(p))))
        out.append((th, tw, slots, P, passes))
    return out


def tiled_many_x8_reference(fn, images, tile, pad, windows_per_pass=16, slots_per_pass=None):
    """Pure-torch restatement of the x8 self-ensemble over an image set and a x4 forward ``fn``: the passes of
    ``tiled_many_x8_passes``; per pass its P windows — filler included — transformed the eight ways of ``x8_transform``
    in runs of ``slots`` transforms, so ``fn`` sees batches of slots P windows, entry (k - k0) P + p, th x tw for k < 4
    and tw x th for k >= 4; the outputs inverse-transformed and summed as seven fp32 adds in k order, times 0.125
    (``tiled_x8_reference``'s arithmetic); and the owned rectangle of every live window's mean copied into its image's
    result.  Nothing is blended.  -> a list of fp32 results, [C', 4H, 4W] or [1, C', 4H, 4W] as the inputs' ranks."""
    xs = _tiled_many_images(list(images), None)
    groups = tiled_many_x8_passes([(v.shape[2], v.shape[3]) for v, _ in xs], tile, pad, windows_per_pass, slots_per_pass)
    tile, pad, _ = _tiled_many_ints(tile, pad, windows_per_pass)
    geo = [tiled_geometry(v.shape[2], v.shape[3], tile, pad) for v, _ in xs]
    outs = [None] * len(xs)
    for th, tw, slots, P, passes in groups:
        for p in passes:
            wins = torch.cat([xs[i][0][:, :, geo[i][4][t][4]:geo[i][4][t][4] + th, geo[i][4][t][5]:geo[i][4][t][5] + tw]
                              for i, t, _ in p], 0)
            acc = None
            for k0 in range(0, 8, slots):
                ys = fn(torch.cat([x8_transform(wins, k) for k in range(k0, k0 + slots)], 0)).float().split(P, 0)
                for k, y in zip(range(k0, k0 + slots), ys):
                    acc = x8_inverse(y, k) if acc is None else acc + x8_inverse(y, k)
            mean = acc * 0.125
            for s, (i, t, live) in enumerate(p):
                if not live:
                    continue
                if outs[i] is None:
                    outs[i] = mean.new_empty((1, mean.shape[1], 4 * xs[i][0].shape[2], 4 * xs[i][0].shape[3]))
                y0, y1, x0, x1, wy, wx = geo[i][4][t]
                outs[i][:, :, 4 * y0:4 * y1, 4 * x0:4 * x1] = mean[s:s + 1, :, 4 * (y0 - wy):4 * (y1 - wy), 4 * (x0 - wx):4 * (x1 - wx)]
    return [o if rank == 4 else o[0] for o, (_, rank) in zip(outs, xs)]


def _tiled_set_x8_passes(sizes, devices, tile, pad, wpp, slots_per_pass):
    """``_tiled_set_passes`` for the self-ensemble: the groups are ``tiled_many_x8_passes``'."""
    m = max(max(s) for s in sizes)
    tile, pad = min(tile, m), min(pad, m)
    groups = tiled_many_x8_passes(sizes, tile, pad, wpp, slots_per_pass)
    return tile, pad, groups, _one_gpu(devices)


def run_rrdbnet_tiled_many_x8(net, images, tile=96, pad=16, windows_per_pass=16, slots_per_pass=None):
    """The x8 self-ensemble of RRDBNet over an image set: ``run_rrdbnet_tiled_x8``'s ensemble per window — pad included,
    eight transforms, inverse transforms summed in k order, times 0.125, the owned rectangle of the mean copied out —
    with ``run_rrdbnet_tiled_many``'s packing: the windows of ALL images share the passes (``tiled_many_x8_passes``),
    grouped by window shape, P = min(max(1, windows_per_pass // slots), windows of the group) windows per pass, each
    pass run 8 / slots times as one batch of slots x P entries of the ordinary inference plan (two plans for non-square
    windows) and chained into the results; only a group's last pass holds filler.  ``windows_per_pass`` counts batch
    entries, so the default pass is the 16 x 128 x 128 batch bench.py measures, where a loop of ``run_rrdbnet_tiled_x8``
    over small images runs slots x P of one image each.  ``images``, the results (fresh fp32 tensors, ranks and order as
    the inputs, no gradient), the pinned slot table (one 24-byte entry per window and side, one non-blocking copy), the
    stream order and the cutting of tile / pad down to the largest image are ``run_rrdbnet_tiled_many``'s.  One launch
    plan per (slots, P, window shape, precision, weight generation), keyed 'tiled_set_x8' — no image size in the key —
    between the table-driven gather-import and stitch-reduce of include/esrgan_hip.h: esr_tile_set_x8.  Bit-identical
    to ``tiled_many_x8_reference(net, ...)``; for one image, to ``run_rrdbnet_tiled_x8(x[None], tile, pad, P, slots)``
    at windows_per_pass = slots x P.  Noise is off whatever ``net.training`` is; the module's mode and every
    ``requires_grad`` are left untouched.  Measured (profiles/set_x8.md, nb = 23, fp16): the device time is that of the
    plan runs — packing two single-window 128 x 128 images into a pass gives 0.977 of the per-image loop, not 0.5, since
    a batch of 8 costs half of 16 — the gain is the host time, the resident bytes and the caller's loop.  Out of scope:
    scales other than 4, blending."""
    slots_per_pass = _x8_slots_arg(slots_per_pass)
    tile, pad, wpp = _tiled_many_ints(tile, pad, windows_per_pass)
    xs = _tiled_many_images(list(images), net.in_nc)
    if not xs:
        return []
    sizes = [(v.shape[2], v.shape[3]) for v, _ in xs]
    tile, pad, groups, dev = _tiled_set_x8_passes(sizes, [v.device for v, _ in xs], tile, pad, wpp, slots_per_pass)
    xin = [v.detach().contiguous().float() for v, _ in xs]
    outs = _run_tiled_set(net, 'tiled_set_x8', E.TileSetX8Ends, groups, xin, sizes, dev,
                          lambda H, W: torch.empty((1, net.out_nc, 4 * H, 4 * W), dtype=torch.float32, device=dev),
                          tile=tile, pad=pad, bgr=0)
    return [o if rank == 4 else o[0] for o, (_, rank) in zip(outs, xs)]


def _tile_item_dtype():
    import numpy as np
    return np.dtype([('nchw', '<u8'), ('H', '<i4'), ('W', '<i4'), ('t', '<i4'), ('live', '<i4')])   # esr_tile_item


def run_rrdbnet_tiled_many(net, images, tile=96, pad=16, windows_per_pass=16):
    """Tiled eval forward of RRDBNet over an image set: ``run_rrdbnet_tiled``'s windows and geometry per image, but the
    windows of ALL images share the passes (``tiled_many_passes``): grouped by window shape, S = min(windows_per_pass,
    windows of the group) per pass, so a folder costs ceil(windows / S) passes per shape where a loop of
    ``run_rrdbnet_tiled`` costs that per image; only a group's last pass holds filler (its last window again, gathered
    but not stitched).  ``images``: a sequence of [C, H, W] or [1, C, H, W] float32 tensors on one GPU, of any sizes ->
    a list of fp32 results [out_nc, 4H, 4W] / [1, out_nc, 4H, 4W], ranks and order as the inputs, without gradient; an
    empty list gives [].  One launch plan per (S, window shape, precision, weight generation) — no image size in the
    key — the ordinary inference plan of batch S between a table-driven gather and stitch (include/esrgan_hip.h:
    esr_tile_many).  The slot table of the whole call (two 24-byte entries per slot: the LR image and the HR result) is
    written into a pinned ring buffer and uploaded with one non-blocking copy; every pass points its two ops at its
    slice.  Everything runs on the current stream without a device synchronisation; the results are fresh tensors.  The
    device holds the plan's activations of S windows plus this call's inputs and outputs.  Bit-identical to
    ``tiled_many_reference(net, ...)``; for one image, to ``run_rrdbnet_tiled(x, tile, pad, windows_per_pass)``.  Noise
    is off whatever ``net.training`` is; the module's mode and every ``requires_grad`` are left untouched.
    Out of scope: scales other than 4, blending.  For 8-bit images in and out see ``run_rrdbnet_images``: the same passes
    with the uint8 conversions fused into the two ends; for the x8 self-ensemble, ``run_rrdbnet_tiled_many_x8``."""
    tile, pad, wpp = _tiled_many_ints(tile, pad, windows_per_pass)
    xs = _tiled_many_images(list(images), net.in_nc)
    if not xs:
        return []
    sizes = [(v.shape[2], v.shape[3]) for v, _ in xs]
    tile, pad, groups, dev = _tiled_set_passes(sizes, [v.device for v, _ in xs], tile, pad, wpp)
    xin = [v.detach().contiguous().float() for v, _ in xs]
    outs = _run_tiled_set(net, 'tiled_many', E.TileManyEnds, groups, xin, sizes, dev,
                          lambda H, W: torch.empty((1, net.out_nc, 4 * H, 4 * W), dtype=torch.float32, device=dev),
                          tile=tile, pad=pad)
    return [o if rank == 4 else o[0] for o, (_, rank) in zip(outs, xs)]


def _tiled_set_passes(sizes, devices, tile, pad, wpp):
    """What a tiled forward over an image set settles before it touches the device, from the images' LR sizes and
    devices and the validated ints -> (tile, pad, groups, device): tile and pad cut down to the largest image, which
    changes no tile and no window; the passes (``tiled_many_passes``, which refuses more than 65535 slots per pass); and
    the one GPU all images are on."""
    m = max(max(s) for s in sizes)
    tile, pad = min(tile, m), min(pad, m)
    groups = tiled_many_passes(sizes, tile, pad, wpp)
    return tile, pad, groups, _one_gpu(devices)


def _one_gpu(devices):
    """The one GPU all images of a tiled forward are on."""
    dev = devices[0]
    for i, d in enumerate(devices):
        if d != dev:
            raise ValueError('image %d is on %s, image 0 on %s: a tiled forward runs on one device' % (i, d, dev))
    if dev.type != 'cuda':
        raise ValueError('the images of a tiled forward are on %s: the HIP path needs tensors on an MI355X; there is '
                         'no CPU fallback' % (dev,))
    return dev


def _run_tiled_set(net, kind, ends, groups, xin, sizes, dev, new_out, img=False, desc=None, **bound):
    """The passes ``groups`` (``tiled_many_passes``) of a tiled forward over the device images ``xin`` of the LR sizes
    ``sizes``, on the current stream -> the results, one ``new_out(H, W)`` per image.  One slot table for the call, the
    gather's entries of every pass of every group, then the stitch's (the 24-byte layout of esr_tile_item), uploaded
    through the net's pinned ring in one non-blocking copy; one plan per group between the engine's ``ends``, keyed
    (kind, S, th, tw, precision, generation) and bound to ``bound`` (tile, pad, ...); every pass runs it on its gather
    slice and its stitch slice.  Groups of ``tiled_many_x8_passes`` (th, tw, slots, P, passes) run the self-ensemble
    instead: the table holds one entry per WINDOW, the plan is keyed (kind, slots, P, th, tw, precision, generation) and
    runs its ``x8_passes`` on every pass's slices between ``E.TileSetX8Ends``; ``img``: the images outside are 8-bit.
    ``desc``: a numpy record array with one descriptor per image (esr_tile_hr_desc) in the place of ``xin``: it travels
    behind the slot table in the same copy, and the gather's entries name the descriptors' device addresses."""
    import numpy as np
    with E.StreamOrder.of(net).call():
        wp = net._weights(dev)
        outs = [new_out(H, W) for H, W in sizes]
        flat = [w for g in groups for p in g[-1] for w in p]
        n = len(flat)
        idx = np.fromiter((w[0] for w in flat), dtype=np.int64, count=n)
        rec = np.zeros(2 * n, dtype=_tile_item_dtype())
        if desc is None:
            rec['nchw'][:n] = np.array([x.data_ptr() for x in xin], dtype=np.uint64)[idx]
        rec['nchw'][n:] = np.array([o.data_ptr() for o in outs], dtype=np.uint64)[idx]
        hw = np.array(sizes, dtype=np.int32)[idx]
        rec['H'][:n] = rec['H'][n:] = hw[:, 0]
        rec['W'][:n] = rec['W'][n:] = hw[:, 1]
        rec['t'][:n] = rec['t'][n:] = np.fromiter((w[1] for w in flat), dtype=np.int32, count=n)
        rec['live'][:n] = rec['live'][n:] = np.fromiter((w[2] for w in flat), dtype=np.int32, count=n)
        rings = net.__dict__.setdefault('_table_rings', {})
        ring = rings.get(dev.index)
        if ring is None:
            ring = rings[dev.index] = E.PinnedRing()
        if desc is None:
            table = ring.upload(rec, dev)
        else:
            # the device tensor first: the gather's entries hold addresses inside it
            table = torch.empty(rec.nbytes + desc.nbytes, dtype=torch.uint8, device=dev)
            rec['nchw'][:n] = (table.data_ptr() + rec.nbytes + idx * desc.dtype.itemsize).astype(np.uint64)
            ring.upload(np.concatenate([rec.view(np.uint8), desc.view(np.uint8)]), dev, out=table)
        isz, stream, at = rec.dtype.itemsize, E.current_stream(), 0
        for th, tw, *per_pass, passes in groups:
            # no H, W in the key: whatever images have this window
            if len(per_pass) == 1:
                S, = per_pass
                plan = _cached_plan(net, (kind, S, th, tw, net.precision, wp.generation),
                                    lambda: E.build_rrdbnet_tiled_many_plan(wp, net.nb, net.in_nc, net.out_nc, S, th, tw,
                                                                            net.precision, dev, net.variant, ends))
            else:
                slots, S = per_pass
                plan = _cached_plan(net, (kind, slots, S, th, tw, net.precision, wp.generation),
                                    lambda: E.build_rrdbnet_tiled_set_x8_plan(wp, net.nb, net.in_nc, net.out_nc, S, th, tw,
                                                                              net.precision, dev, net.variant, slots, img))
            plan.bind(**bound)
            for _ in passes:
                plan.run(table[at * isz:(at + S) * isz], table[(n + at) * isz:(n + at + S) * isz], stream)
                at += S
    return outs


def _images_u8(images):
    """The images of ``run_rrdbnet_images`` / ``images_reference`` as a list: uint8 tensors [H, W, 3] with pixels."""
    images = list(images)
    for i, x in enumerate(images):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8:
            raise ValueError('image %d of forward_images must be a torch.uint8 tensor, got %s'
                             % (i, x.dtype if isinstance(x, torch.Tensor) else type(x).__name__))
        if x.dim() != 3:
            raise ValueError('image %d of forward_images must be [H, W, 3] (HWC), got rank %d: %s' % (i, x.dim(), tuple(x.shape)))
        if x.shape[2] != 3:
            raise ValueError('image %d of forward_images must be [H, W, 3] (HWC): its last dimension is %d' % (i, x.shape[2]))
        if x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError('image %d of a tiled forward has no pixels: shape %s' % (i, tuple(x.shape)))
    return images


def images_reference(fn, images, tile, pad, windows_per_pass=16, bgr=False):
    """Pure-torch restatement of ``run_rrdbnet_images`` and a x4 forward ``fn``, on any device: every uint8 [H, W, 3]
    image -> NCHW float32 RGB, ``float32(v) / 255`` as a true division (bit-identical, for all 256 values, to the
    ``astype(float64) / 255 -> float32`` of the reference's inference script); ``tiled_many_reference(fn, ...)``;
    ``(y.clamp(0, 1) * 255.0).round()`` -> uint8 [4H, 4W, 3].  ``bgr``: the channel order in memory is B, G, R on both
    ends, else R, G, B; ``fn`` sees RGB either way.  The 256 quotients are divided once, on the CPU, and looked up: on
    a GPU torch divides by a Python scalar as a multiplication by its reciprocal, which differs for 126 of them."""
    images = _images_u8(images)
    lut = torch.arange(256, dtype=torch.float32) / 255.0
    xs = [lut.to(x.device)[(x.flip(2) if bgr else x).permute(2, 0, 1).long()] for x in images]
    ys = tiled_many_reference(fn, xs, tile, pad, windows_per_pass)
    outs = [(y.clamp(0, 1) * 255.0).round().to(torch.uint8).permute(1, 2, 0) for y in ys]
    return [(o.flip(2) if bgr else o).contiguous() for o in outs]


def images_x8_reference(fn, images, tile, pad, windows_per_pass=16, slots_per_pass=None, bgr=False):
    """``images_reference`` with ``tiled_many_x8_reference`` in the middle: the same look-up-table division on the way
    in, the self-ensemble's fp32 mean per window, the same ``(y.clamp(0, 1) * 255.0).round()`` on the way out — the
    quantisation of ``tiled_many_x8_reference``'s floats."""
    images = _images_u8(images)
    lut = torch.arange(256, dtype=torch.float32) / 255.0
    xs = [lut.to(x.device)[(x.flip(2) if bgr else x).permute(2, 0, 1).long()] for x in images]
    ys = tiled_many_x8_reference(fn, xs, tile, pad, windows_per_pass, slots_per_pass)
    outs = [(y.clamp(0, 1) * 255.0).round().to(torch.uint8).permute(1, 2, 0) for y in ys]
    return [(o.flip(2) if bgr else o).contiguous() for o in outs]


def run_rrdbnet_images(net, images, tile=96, pad=16, windows_per_pass=16, bgr=False, x8=False, slots_per_pass=None):
    """``run_rrdbnet_tiled_many`` with 8-bit ends: ``images`` is a sequence of ``torch.uint8`` tensors [H, W, 3] (HWC, as
    PIL and cv2 hold an image), of any sizes, on one GPU -> a list of fresh uint8 device tensors [4H, 4W, 3], in input
    order, without gradient; an empty list gives [].  ``bgr=False``: R, G, B in memory on both ends (PIL); ``bgr=True``:
    B, G, R on both ends (cv2.imread / imwrite, the reference's scripts, ``metrics.device_tensor2img``,
    ``TrainSet(bgr=True)``).  The reference's inference-script conversions are fused into the two ends
    (include/esrgan_hip.h: esr_tile_img): the gather reads the bytes and divides, ``float32(v) / 255.0f`` correctly
    rounded — bit-identical to the script's float64 division rounded to float32, which a multiplication by 1/255 is not —
    and the stitch writes ``rint(clamp(v, 0, 1) * 255)`` (``tensor2img``'s rounding; non-finite outputs: unspecified).  A
    folder costs 3 bytes up and 48 bytes down and resident per LR pixel where the float32 ends cost 12 and 192, and
    nothing is computed per pixel on the host.  Windows, passes, filler, the grouping by window shape, the 65535-slot
    limit and the cutting of tile / pad down to the largest image are ``run_rrdbnet_tiled_many``'s; so is the plan in
    between: one per (S, window shape, precision, weight generation), keyed 'tiled_img' — no image size and no ``bgr``
    in the key; tile, pad and bgr are set on the two ops per run.  ``tile`` >= the largest image side makes every
    window a whole image: that is the whole-image route.  Non-contiguous images are made contiguous.  Everything runs on
    the current stream without a device synchronisation.  Bit-identical to ``images_reference(net, ...)`` and to
    ``device_tensor2img`` of ``run_rrdbnet_tiled_many``'s results.  Noise is off whatever ``net.training`` is; the
    module's mode and every ``requires_grad`` are left untouched.
    ``x8=True`` is the self-ensemble per window with the same 8-bit ends (``run_rrdbnet_tiled_many_x8``'s passes, with
    ``slots_per_pass``; include/esrgan_hip.h: esr_tile_set_x8, img = 1): the gather-import divides, the last k range of
    the stitch-reduce quantises the mean, and between the ranges the partial sums stay in an fp32 buffer of the plan, P
    windows large (none when all eight slots run in one pass).  Keyed 'tiled_set_x8_img'; bit-identical to
    ``images_x8_reference(net, ...)`` and to the quantisation of ``run_rrdbnet_tiled_many_x8``'s floats.
    Out of scope: scales other than 4, 16-bit or alpha images, CPU or numpy inputs, blending."""
    slots_per_pass = _x8_slots_arg(slots_per_pass, x8)
    tile, pad, wpp = _tiled_many_ints(tile, pad, windows_per_pass)
    images = _images_u8(images)
    if net.in_nc != 3 or net.out_nc != 3:
        raise ValueError('forward_images takes and gives 3-channel 8-bit images: this net has in_nc = %d, out_nc = %d'
                         % (net.in_nc, net.out_nc))
    if not images:
        return []
    sizes = [(x.shape[0], x.shape[1]) for x in images]
    if x8:
        tile, pad, groups, dev = _tiled_set_x8_passes(sizes, [x.device for x in images], tile, pad, wpp, slots_per_pass)
        kind, ends = 'tiled_set_x8_img', E.TileSetX8Ends
    else:
        tile, pad, groups, dev = _tiled_set_passes(sizes, [x.device for x in images], tile, pad, wpp)
        kind, ends = 'tiled_img', E.TileImgEnds
    xin = [x.detach().contiguous() for x in images]
    return _run_tiled_set(net, kind, ends, groups, xin, sizes, dev,
                          lambda H, W: torch.empty((4 * H, 4 * W, 3), dtype=torch.uint8, device=dev),
                          img=bool(x8), tile=tile, pad=pad, bgr=1 if bgr else 0)


def run_rrdbnet_evaluate(net, lr_images, hr_images, tile=96, pad=16, windows_per_pass=16, bgr=False, crop=None,
                         x8=False, slots_per_pass=None):
    """codes/test.py:49-110 for one image set: ``run_rrdbnet_images`` on ``lr_images``, then
    ``metrics.device_set_metrics`` on its results against ``hr_images`` (uint8 [4H, 4W, 3] device tensors, one per LR
    image, channel order as ``bgr`` says) -> ``(sr_images, result)``: the uint8 results of ``run_rrdbnet_images`` and a
    ``metrics.SetMetricsResult`` whose ``read()`` gives (psnr, ssim, psnr_y, ssim_y) per image.  ``crop=None`` cuts
    ``net.upscale`` pixels from every side (test.py:75).  Sizes, types and the crop are checked before anything is
    launched; everything is queued on the current stream and nothing synchronises before ``result.read()``.  ``x8`` and
    ``slots_per_pass`` are ``run_rrdbnet_images``': the score of the self-ensemble."""
    from . import metrics as M
    slots_per_pass = _x8_slots_arg(slots_per_pass, x8)
    lr, hr = _images_u8(lr_images), _images_u8(hr_images)
    if len(lr) != len(hr):
        raise ValueError('evaluate_images compares equally many images: %d lr, %d hr' % (len(lr), len(hr)))
    s = net.upscale
    for i, (a, b) in enumerate(zip(lr, hr)):
        if (b.shape[0], b.shape[1]) != (s * a.shape[0], s * a.shape[1]):
            raise ValueError('hr image %d of evaluate_images must be [%d, %d, 3], x%d of its lr image: got %s'
                             % (i, s * a.shape[0], s * a.shape[1], s, tuple(b.shape)))
        if b.device != a.device:
            raise ValueError('hr image %d is on %s, its lr image on %s' % (i, b.device, a.device))
    crop = M._set_crop([(b.shape[0], b.shape[1]) for b in hr], s if crop is None else crop)
    sr = run_rrdbnet_images(net, lr, tile, pad, windows_per_pass, bgr, x8, slots_per_pass)
    return sr, M.device_set_metrics(sr, hr, crop, bgr)


# ---- a generator scored from HR images alone: the LR is made in the gather (include/esrgan_hip.h: esr_tile_hr) ---------
def _hr_images(net, hr_images):
    """The HR images of ``run_rrdbnet_hr_images`` as a list, checked without a device: what ``_images_u8`` refuses, HR
    sides below 4, nets that are not 3 -> 3."""
    images = _images_u8(hr_images)
    for i, x in enumerate(images):
        if x.shape[0] < 4 or x.shape[1] < 4:
            raise ValueError('hr image %d of forward_hr_images is %d x %d: below 4 pixels a side there is no x4 LR image'
                             % (i, x.shape[0], x.shape[1]))
    if net.in_nc != 3 or net.out_nc != 3:
        raise ValueError('forward_hr_images takes and gives 3-channel 8-bit images: this net has in_nc = %d, out_nc = %d'
                         % (net.in_nc, net.out_nc))
    return images


def _hr_desc_dtype():
    import ctypes as C
    import numpy as np
    from . import _lib as L
    dt = np.dtype([(n, {C.c_void_p: '<u8', C.c_int32: '<i4'}[t]) for n, t in L.esr_tile_hr_desc._fields_], align=True)
    assert dt.itemsize == C.sizeof(L.esr_tile_hr_desc) == 64
    return dt


def hr_lr_reference(hr_images, bgr=False):
    """The two float images ``LRHRDataset.__getitem__`` makes of an HR image when ``dataroot_LR`` is null and the phase is
    not 'train' (codes/data/LRHR_dataset.py:44-125), restated with torch on the images' device, per uint8 [H, W, 3]
    image: ``data.modcrop(., 4)``, ``float32(v) / 255`` as a true division (the look-up table of ``images_reference``),
    R, G, B order; the LR is the resample of ``data.batch_reference`` — the tables of ``data.resample_tables`` as sums
    over the taps, H pass then W pass — in the kernels' order and rounding (``data.table_resample_fused``: taps
    ascending, one fused multiply-add each; ``data.table_resample``'s products and torch's summation order round
    differently in most values, by an ulp), not quantised and not clamped.
    -> (lr [3, H // 4, W // 4] float32 list, hr [3, 4 (H // 4), 4 (W // 4)] float32 list)."""
    from . import data as D
    images = _images_u8(hr_images)
    lut = torch.arange(256, dtype=torch.float32) / 255.0
    hrs = [lut.to(x.device)[D.modcrop((x.flip(2) if bgr else x).permute(2, 0, 1), 4).long()] for x in images]
    return [D.table_resample_fused(h, 4) for h in hrs], hrs


def hr_images_reference(fn, hr_images, tile, pad, windows_per_pass=16, bgr=False):
    """Pure-torch restatement of ``run_rrdbnet_hr_images`` and a x4 forward ``fn``, on any device: the LR images of
    ``hr_lr_reference``, ``tiled_many_reference(fn, ...)`` on them, and ``images_reference``'s quantisation
    ``(y.clamp(0, 1) * 255.0).round()`` -> uint8 [4 (H // 4), 4 (W // 4), 3] in the inputs' channel order."""
    lrs, _ = hr_lr_reference(hr_images, bgr)
    ys = tiled_many_reference(fn, lrs, tile, pad, windows_per_pass)
    outs = [(y.clamp(0, 1) * 255.0).round().to(torch.uint8).permute(1, 2, 0) for y in ys]
    return [(o.flip(2) if bgr else o).contiguous() for o in outs]


def run_rrdbnet_hr_images(net, hr_images, tile=96, pad=16, windows_per_pass=16, bgr=False):
    """``run_rrdbnet_images`` of the LR images the reference's dataset makes of ground-truth images alone
    (codes/data/LRHR_dataset.py:44-125 with ``dataroot_LR`` null, phase 'val' / 'test': ``modcrop(HR, 4)``, then
    ``imresize_np(HR, 1 / 4)`` on the float image — neither quantised nor clamped).  ``hr_images``: a sequence of
    ``torch.uint8`` tensors [H, W, 3] of any sizes >= 4 a side on one GPU -> a list of fresh uint8 device tensors
    [4 (H // 4), 4 (W // 4), 3], in input order, without gradient; an empty list gives [].  No LR image ever exists: the
    gather of every pass (include/esrgan_hip.h: esr_tile_hr) cuts each window straight out of the HR bytes through the
    whole image's MATLAB-bicubic tables — ``float32(v) / 255.0f`` per sample, H pass then W pass, taps ascending in fp32,
    the bits of ``data.imresize(hr_float, 1 / 4)`` — and the stitch is ``run_rrdbnet_images``'.  A modcropped image is
    read through its row pitch, not copied.  Windows, passes, filler, the grouping by window shape and the cutting of
    tile / pad down to the largest LR image are ``run_rrdbnet_tiled_many``'s on the LR sizes; one plan per (S, window
    shape, precision, weight generation), keyed 'tiled_hr' — no image size and no ``bgr`` in the key.  The per-image
    descriptors (HR bytes, pitch, size, tables) go up behind the slot table in the same non-blocking copy; the tables are
    cached on the device per (length, scale).  Everything runs on the current stream without a device synchronisation.
    Bit-identical to ``metrics.device_tensor2img`` of ``run_rrdbnet_tiled_many`` on ``data.imresize`` of the float
    images.  Refused before the device is touched: what ``run_rrdbnet_images`` refuses, HR sides below 4, nets that are
    not 3 -> 3, more than one device, CPU tensors.
    Not offered: the x8 self-ensemble on this route (there is no such keyword), scales other than 4, and writing LR or Bic
    image files (the reference's scripts/generate_mod_LR_bic.py resamples 0..255 values and lets ``cv2.imwrite`` round:
    other numbers than the dataset's)."""
    import numpy as np
    from . import data as D
    tile, pad, wpp = _tiled_many_ints(tile, pad, windows_per_pass)
    images = _hr_images(net, hr_images)
    if not images:
        return []
    sizes = [(x.shape[0] // 4, x.shape[1] // 4) for x in images]
    tile, pad, groups, dev = _tiled_set_passes(sizes, [x.device for x in images], tile, pad, wpp)
    xin = [x.detach().contiguous() for x in images]
    with torch.cuda.device(dev):
        desc, tables = np.zeros(len(xin), dtype=_hr_desc_dtype()), []        # `tables` keeps them referenced until queued
        for i, (x, (H, W)) in enumerate(zip(xin, sizes)):
            (wy, iy, oh), (wx, ix, ow) = D.device_tables(4 * H, 0.25, dev), D.device_tables(4 * W, 0.25, dev)
            assert (oh, ow) == (H, W) and wy.shape == iy.shape and wx.shape == ix.shape
            tables.append((wy, iy, wx, ix))
            d = desc[i]
            d['hr'], d['pitch'], d['hr_h'], d['hr_w'] = x.data_ptr(), x.shape[1], 4 * H, 4 * W
            d['wy'], d['iy'], d['taps_y'] = wy.data_ptr(), iy.data_ptr(), wy.shape[1]
            d['wx'], d['ix'], d['taps_x'] = wx.data_ptr(), ix.data_ptr(), wx.shape[1]
        outs = _run_tiled_set(net, 'tiled_hr', E.TileHrEnds, groups, None, sizes, dev,
                              lambda H, W: torch.empty((4 * H, 4 * W, 3), dtype=torch.uint8, device=dev),
                              desc=desc, tile=tile, pad=pad, bgr=1 if bgr else 0)
    del tables, xin
    return outs


def _modcropped(images):
    """The images cut to multiples of 4 a side: the image itself where nothing is cut, else a contiguous copy."""
    return [x if (x.shape[0] % 4 == 0 and x.shape[1] % 4 == 0)
            else x[:x.shape[0] - x.shape[0] % 4, :x.shape[1] - x.shape[1] % 4].contiguous() for x in images]


def run_rrdbnet_evaluate_hr(net, hr_images, tile=96, pad=16, windows_per_pass=16, bgr=False, crop=None):
    """codes/test.py:49-110 for a folder of ground-truth images alone: ``run_rrdbnet_hr_images``, then
    ``metrics.device_set_metrics`` of its results against the modcropped HR images -> ``(sr_images, result)`` as
    ``run_rrdbnet_evaluate``.  ``crop=None`` cuts ``net.upscale`` pixels from every side.  The set metric's items have
    no row pitch: only the images that modcrop cuts are copied, cropped and contiguous, on the device.  Types, sizes and
    the crop are checked before anything is launched; nothing synchronises before ``result.read()``.  These are the
    reference's numbers for the HR-only configuration; ``run_rrdbnet_evaluate`` on stored 8-bit LR files gives others,
    because a stored LR has been rounded.  Not offered: ``x8``, scales other than 4."""
    from . import metrics as M
    _tiled_many_ints(tile, pad, windows_per_pass)
    images = _hr_images(net, hr_images)
    crop = M._set_crop([(x.shape[0] - x.shape[0] % 4, x.shape[1] - x.shape[1] % 4) for x in images],
                       net.upscale if crop is None else crop)
    sr = run_rrdbnet_hr_images(net, images, tile, pad, windows_per_pass, bgr)
    return sr, M.device_set_metrics(sr, _modcropped(images), crop, bgr)
