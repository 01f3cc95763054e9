"""Launch plans (forward + backward) for the two feed-forward conv nets of the ESRGAN+ train step:
``Discriminator_VGG_128`` (codes/models/modules/architecture.py:87-129) and the VGG19 feature
extractor (architecture.py:279-307; body = torchvision cfg 'E' ``features[:35]``).

Same mechanics as engine.py: G32 buffers, fused-conv launches, one ``esr_run_ops`` per pass.
Convs keep their LeakyReLU / ReLU in the epilogue; BatchNorm2d runs as stats -> finalize -> apply
passes over the conv output; the backward applies activation masks inside the producing kernels
(conv epilogue ``out2``, BN backward, max-pool backward).
"""
import os
from collections import namedtuple

import torch

from . import _lib as L
from . import engine as E

BN_MOMENTUM, BN_EPS = 0.1, 1e-5      # nn.BatchNorm2d defaults (block.py:31)
# ESR_FUSE_BN=0: the five-launch BatchNorm of round 3 (stats, finalize, apply / reduce, final, apply) for A/B runs
def fuse_bn():
    return os.environ.get('ESR_FUSE_BN', '1') != '0'


class _Lease(object):
    def __init__(self, plan):
        self.plan = plan
        plan.busy = True

    def release(self):
        if self.plan is not None:
            self.plan.busy = False
            self.plan = None

    def __del__(self):
        self.release()


def s2_ksplit(B, wo, ho, cin, cout, dt_e):
    """K split of a 4x4/s2 conv that leaves a square map of 4 / 8 / 16 columns (the discriminators' deep layers:
    include/esrgan_hip.h, esr_conv.ksplit): enough workgroups to fill the chip, at least two K steps each; 0 = the
    plain one-image-per-tile launch (other shapes, fp32, ESR_S2_SPLIT=0)."""
    if dt_e != L.ESR_F16 or wo != ho or wo not in (4, 8, 16) or B < 2 or os.environ.get('ESR_S2_SPLIT', '1') == '0':
        return 0
    nchunks = (cin + 15) // 16
    per_tile = (32 // wo) * (2 if wo <= 4 else 1)
    tyn = 1 if wo <= 4 else (wo + 7) // 8
    base = ((B + per_tile - 1) // per_tile) * tyn * ((cout + 127) // 128)
    k = 1
    while k * 2 <= nchunks // 2 and k * 2 * base <= 256:
        k *= 2
    return k if k >= 2 else 0


def _lin(mode, B_, I, O, act, **kw):
    o = L.esr_linear()
    o.mode, o.B, o.I, o.O, o.act = mode, B_, I, O, act
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _pad32(c):
    return ((c + 31) // 32) * 32


class BwdPass:
    """One backward launch list over a plan's saved activations with its own scratch buffers."""

    def __init__(self):
        self.bwd = L.OpList()
        self.bufs, self.keep = [], []   # G32 buffers / plain tensors the launches point at
        self.gy_tensor = None           # fp32 tensor the upstream gradient is copied (or written by the loss kernel) into
        self.gx_tensor = None           # fp32 NCHW gradient w.r.t. the input image
        self.gx_op = None               # index in bwd of the layout op that exports it (run_pass_into rebinds its target)
        self.sums_b = None              # fp64 BatchNorm backward sums, zeroed before every run
        self.has_bn = True              # False: no launch reads sums_b
        self.grad_flat = None           # fp32 parameter gradients, flat in pspec order (None: parameters frozen)
        self.grad_views = None          # [(numel, shape)] of the parameters inside grad_flat
        self.param_views = self.param_list = None    # train step: views of grad_flat and the parameters whose .grad they are
        self.tapmajor = self.wgrad_arena = None      # fp16 weight gradients: E.TapMajorGrads staging; partial sums of the
                                                     # deterministic reduction


class SeqPlan(BwdPass):
    """Forward/backward launch lists of a conv -> [bn] -> act -> [pool] chain (+ optional linear
    head) for one input shape."""

    def __init__(self):
        super().__init__()
        self.fwd = L.OpList()
        self.busy = False               # leased to a forward whose backward has not run yet
        self.in_op = None               # index in fwd of the layout op that imports the input
        self.out_tensor = None          # fp32 output (NCHW features, or the head's [B, O2])
        self.sums_f = None              # fp64 BatchNorm forward sums, zeroed before every training forward
        self.bn_layers = []
        self.second = None              # BwdPass of a dual plan (build_seq_plan(dual=...)): the G step's input-gradient pass
        self.restat = None              # OpList replaying the BatchNorm running-statistics updates (dual plans)
        self.fwd_half = self.restat1 = None  # split_forward_groups: [group 0, group 1] forward lists over a pair's halves, and
                                             # the running-statistics update the early half owes
        self.restat0 = None             # group0_restat: the running-statistics update of ONE more call on group 0
        self.own_dp = self.own_head = None   # per-call weights: this plan's own input-gradient pack / head weights
        self.graph, self.x_static = False, None      # hipGraph replay, the input staged in x_static
        self.packs = self.keep_x = None      # kept alive with the plan: the (WeightPack, DgradPack) the lists point into,
                                             # the input tensor(s) of the forward in flight


# Layer records of the forward, read by the backward.  SaveRec: a residual source (no launch).  ShuffleRec / PoolRec:
# input and output buffers; channels and map as the launch states them.
SaveRec = namedtuple('SaveRec', 'tag')
ShuffleRec = namedtuple('ShuffleRec', 'x y ch h w')
PoolRec = namedtuple('PoolRec', 'x y ch h w')


class ConvRec:
    """Conv layer: input x (cin, hin x win), output y (cout, h x w) after the activation `act`."""
    __slots__ = ('key', 'x', 'cin', 'hin', 'win', 'y', 'cout', 'h', 'w', 'ks', 'st', 'act',
                 'ups', 'res', 'alpha',       # nearest x2 in the load; residual tag and the conv's scale in front of the add (else 1)
                 'bn', 'ibn', 'c',            # BatchNorm parameters (None: no norm), its index, the conv output it reads
                 'base', 'sums_f', 'mean', 'invstd')      # element offset of its statistics; pointers to sums / mean / 1/std

    def __init__(self, s, x, cin, hin, win, y, h, w):
        self.key, self.cout, self.ks, self.st, self.act = s['conv'], s['cout'], s['ks'], s['stride'], s['act']
        self.x, self.cin, self.hin, self.win, self.y, self.h, self.w = x, cin, hin, win, y, h, w
        self.bn, self.ups, self.res = s.get('bn'), bool(s.get('ups')), s.get('res')
        self.alpha = float(s.get('alpha', 1.0)) if self.res is not None else 1.0
        self.ibn = self.c = self.base = self.sums_f = self.mean = self.invstd = None


def _epilogue_act(r):
    """The activation a record's own conv epilogue applied: the one whose mask its consumer's backward must apply."""
    return r.act if isinstance(r, ConvRec) and r.bn is None else L.ACT_NONE


class _BwdCursor:
    """Where the emission of one backward pass stands."""

    def __init__(self, Q, Bb, gb):
        self.Q, self.Bb, self.gb = Q, Bb, gb    # the pass, images it covers, statistics groups it sees
        self.params_grad, self.poff = {}, {}    # '<layer>' -> (dw, db) pointers; '<name>' -> element offset in grad_flat
        self.gcur, self.masked = None, False    # G32 gradient w.r.t. the current layer's OUTPUT (post-activation); True
                                                # when it already is the gradient w.r.t. the producing conv's pre-activation
        self.skips = {}          # residual tag -> gradient buffers that flow back to the saved tensor over the skip


class SeqBuilder:
    """Emits one SeqPlan: the forward steps in order, then ``backward`` once per pass over the saved activations."""

    def __init__(self, spec, wp, dp, pspec, B, H, W, dtype, dev, training, input_affine, head, groups):
        self.spec, self.wp, self.dp, self.pspec = spec, wp, dp, pspec
        self.B, self.H, self.W, self.dtype, self.dev = B, H, W, dtype, dev
        self.dt_e, _, self.cpg = E._dt(dtype)
        self.training, self.input_affine, self.head, self.groups = training, input_affine, head, groups
        self.nbn = sum(1 for s in spec if s.get('bn'))
        self.maxc = max([s['cout'] for s in spec if 'conv' in s] + [1])
        self.plan = SeqPlan()
        self.plan.grad_views = self.grad_views = [(t.numel(), tuple(t.shape)) for _, t in pspec]
        self.recs, self.bn_recs, self.saved = [], [], {}     # layer records; those with BatchNorm; residual sources by tag
        self.cur = self.ch = self.h = self.w = None     # forward cursor: buffer, channels, map
        self.stats = self.F_ = self.H1 = None           # BatchNorm mean | invstd ([groups][C] each); head input / hidden
        self.lin_dims = None                            # head: (flattened features, hidden units, outputs)

    def buf(self, Q, Bb, C_, h, w):
        return E.new_buf(Q.bufs, Bb, C_, h, w, self.dtype, self.dev)

    def stat_sums(self, dtype):
        return torch.zeros(max(self.nbn, 1) * 2 * self.maxc * self.groups, dtype=dtype, device=self.dev)

    def ksplit(self, c, keep, B, r, transposed=False):
        """Split K of c, the 4x4/s2 conv of record r or (transposed) the conv of its input gradient, where s2_ksplit says
        so: the fp32 slabs of the partial sums, one per split over c's output, go into `keep`.  Returns the split
        (0: plain launch)."""
        kch, nch, out_h, out_w = (r.cout, r.cin, r.hin, r.win) if transposed else (r.cin, r.cout, r.h, r.w)
        ksp = s2_ksplit(B, r.w, r.h, kch, nch, self.dt_e) if (r.st == 2 and r.ks == 4) else 0
        if ksp:
            ws = torch.empty(ksp * B * out_h * out_w * _pad32(nch), dtype=torch.float32, device=self.dev)
            keep.append(ws)
            c.ksplit, c.split_ws = ksp, ws.data_ptr()
        return ksp

    def bn_op(self, r, mode, b=None, g=None, gx=None):
        """One BatchNorm launch of conv record r.  Forward modes cover the batch and read r's forward sums; backward
        modes cover the images, statistics groups and sums of the backward pass at cursor b."""
        o = L.esr_bn()
        fwd_op = mode in (L.BN_STATS, L.BN_FINALIZE, L.BN_APPLY, L.BN_RESTAT, L.BN_FIN_APPLY)
        o.dtype, o.mode, o.B, o.C, o.H, o.W = self.dt_e, mode, (self.B if fwd_op else b.Bb), r.cout, r.h, r.w
        o.groups = self.groups if fwd_op else b.gb
        if mode in (L.BN_FINALIZE, L.BN_RESTAT, L.BN_FIN_APPLY) and self.training and r.bn.get('nbt') is not None:
            o.num_batches_tracked = r.bn['nbt'].data_ptr()
        o.training, o.act, o.momentum, o.eps = int(self.training), r.act, BN_MOMENTUM, BN_EPS
        o.x, o.y = r.c.view(0, r.cout), r.y.view(0, r.cout)
        if g is not None:
            o.g = g.view(0, r.cout)
        if gx is not None:
            o.gx = gx.view(0, r.cout)
        o.sums, o.mean, o.invstd = (r.sums_f if fwd_op else b.Q.sums_b.data_ptr() + 8 * r.base), r.mean, r.invstd
        o.gamma, o.beta = r.bn['weight'].data_ptr(), r.bn['bias'].data_ptr()
        o.running_mean, o.running_var = r.bn['rm'].data_ptr(), r.bn['rv'].data_ptr()
        return o

    # ---------------------------------------------------------------- forward
    def forward_input(self):
        P, cin0 = self.plan, self.spec[0]['cin']
        xin = self.buf(P, self.B, cin0, self.H, self.W)
        P.in_op = E.layout_op(P.fwd, self.dt_e, self.B, xin, cin0, 1, affine=self.input_affine)
        P.sums_f = self.stat_sums(torch.float64)
        self.stats = self.stat_sums(torch.float32)
        P.keep.append(self.stats)
        self.cur, self.ch, self.h, self.w = xin, cin0, self.H, self.W

    def forward_layers(self):
        steps = (('save', self.fwd_save), ('shuffle', self.fwd_shuffle), ('pool', self.fwd_pool), ('conv', self.fwd_conv))
        for s in self.spec:
            next((step for key, step in steps if key in s), self.fwd_conv)(s)     # (no known key: KeyError('conv'))

    def fwd_save(self, s):
        self.saved[s['save']] = (self.cur, self.ch)
        self.recs.append(SaveRec(s['save']))

    def fwd_map(self, rec_type, mode, ch, h, w, hy, wy):
        """Pool-kernel launch from the current tensor into a new [ch, hy, wy] one; the launch states the map h x w."""
        y = self.buf(self.plan, self.B, ch, hy, wy)
        pl = L.esr_pool()
        pl.dtype, pl.mode, pl.B, pl.C, pl.H, pl.W = self.dt_e, mode, self.B, ch, h, w
        pl.x, pl.y = self.cur.view(0, self.ch), y.view(0, ch)
        self.plan.fwd.add(L.OP_POOL, 'pool', pl)
        self.recs.append(rec_type(self.cur, y, ch, h, w))
        self.cur, self.ch, self.h, self.w = y, ch, hy, wy

    def fwd_shuffle(self, s):
        if s['shuffle'] != 2 or self.ch % (4 * self.cpg):
            raise L.HipExtensionError('pixel shuffle: factor 2 on a multiple of %d channels' % (4 * self.cpg))
        self.fwd_map(ShuffleRec, L.POOL_SHUFFLE, self.ch // 4, self.h, self.w, 2 * self.h, 2 * self.w)

    def fwd_pool(self, s):
        self.fwd_map(PoolRec, 0, self.ch, self.h // 2, self.w // 2, self.h // 2, self.w // 2)

    def fwd_conv(self, s):
        key, ks, st, pad = s['conv'], s['ks'], s['stride'], (s['ks'] - 1) // 2
        ho, wo = (self.h + 2 * pad - ks) // st + 1, (self.w + 2 * pad - ks) // st + 1
        if s.get('ups'):
            ho, wo = 2 * self.h, 2 * self.w
        r = ConvRec(s, self.cur, self.ch, self.h, self.w, self.buf(self.plan, self.B, _pad32(s['cout']), ho, wo), ho, wo)
        if (r.ups or r.res is not None) and (r.bn is not None or ks != 3 or st != 1
                                             or (r.res is not None and r.act != L.ACT_NONE)):
            raise L.HipExtensionError('conv %s: up-sampling / residual epilogues are for plain 3x3 stride-1 convs' % key)
        (self.fwd_conv_plain if r.bn is None else self.fwd_conv_bn)(r)
        self.recs.append(r)
        self.cur, self.ch, self.h, self.w = r.y, r.cout, ho, wo

    def fwd_conv_plain(self, r):
        c = E._conv(self.dt_e, self.B, r.h, r.w, r.x.view(0), r.cin, r.y.view(0), self.wp.entries[r.key], r.act,
                    stride=r.st, upsample=1 if r.ups else 0)
        if r.res is not None:
            src, src_ch = self.saved[r.res]
            assert src_ch == r.cout and (src.H, src.W) == (r.h, r.w), 'residual source of %s has another shape' % r.key
            c.res1, c.alpha = src.view(0, r.cout), r.alpha
        self.ksplit(c, self.plan.keep, self.B, r)
        self.plan.fwd.add_conv(c)

    def fwd_conv_bn(self, r):
        P, ng = self.plan, self.maxc * self.groups
        r.ibn, r.c, r.base = len(self.bn_recs), self.buf(P, self.B, _pad32(r.cout), r.h, r.w), len(self.bn_recs) * 2 * ng
        r.sums_f = P.sums_f.data_ptr() + 8 * r.base
        r.mean, r.invstd = self.stats.data_ptr() + 4 * r.base, self.stats.data_ptr() + 4 * (r.base + ng)
        cv = E._conv(self.dt_e, self.B, r.h, r.w, r.x.view(0), r.cin, r.c.view(0), self.wp.entries[r.key], L.ACT_NONE,
                     stride=r.st)
        fused = self.training and fuse_bn()
        ksp = self.ksplit(cv, P.keep, self.B, r)
        if ksp and fused:
            # deep stride-2 layer: packed tiles + split K; its finishing pass also takes the BatchNorm statistics
            cv.stat_sums, cv.stat_groups, cv.stat_C = r.sums_f, self.groups, r.cout
        P.fwd.add_conv(cv)
        if fused:
            # statistics pass (unless the conv's finishing pass took them), then ONE pass that finalizes and
            # applies (ESR_BN_FIN_APPLY)
            modes = ([] if ksp else [L.BN_STATS]) + [L.BN_FIN_APPLY]
        else:
            modes = ([L.BN_STATS] if self.training else []) + [L.BN_FINALIZE, L.BN_APPLY]
        for mode in modes:
            P.fwd.add(L.OP_BN, 'bn', self.bn_op(r, mode))
        P.bn_layers.append(r.bn)
        self.bn_recs.append(r)

    def forward_exit(self):
        P, B, head, f32 = self.plan, self.B, self.head, dict(dtype=torch.float32, device=self.dev)
        if head is None:
            P.out_tensor = torch.empty(B, self.ch, self.h, self.w, **f32)
            E.layout_op(P.fwd, self.dt_e, B, self.cur, self.ch, 0, nchw=P.out_tensor.data_ptr())
            return
        I1, O1, O2 = self.lin_dims = self.ch * self.h * self.w, head['w1'].shape[0], head['w2'].shape[0]
        self.F_, self.H1 = torch.empty(B, I1, **f32), torch.empty(B, O1, **f32)
        P.out_tensor = torch.empty(B, O2, **f32)
        P.keep += [self.F_, self.H1]
        E.layout_op(P.fwd, self.dt_e, B, self.cur, self.ch, 0, nchw=self.F_.data_ptr())
        P.fwd.add(L.OP_LINEAR, 'linear', _lin(0, B, I1, O1, L.ACT_LRELU, x=self.F_.data_ptr(), w=head['w1'].data_ptr(),
                                              b=head['b1'].data_ptr(), y=self.H1.data_ptr()))
        P.fwd.add(L.OP_LINEAR, 'linear', _lin(0, B, O1, O2, L.ACT_NONE, x=self.H1.data_ptr(), w=head['w2'].data_ptr(),
                                              b=head['b2'].data_ptr(), y=P.out_tensor.data_ptr()))

    # ---------------------------------------------------------------- backward
    def backward(self, Q, Bb, want_wgrad):
        """Backward launch list over the first Bb images into the BwdPass / SeqPlan Q (own scratch buffers)."""
        b = self.bwd_begin(Q, Bb, want_wgrad)
        self.bwd_entry(b)
        steps = {ShuffleRec: self.bwd_shuffle, PoolRec: self.bwd_pool, ConvRec: self.bwd_conv}
        for li in range(len(self.recs) - 1, -1, -1):
            if type(self.recs[li]) in steps:
                steps[type(self.recs[li])](b, li)
        self.bwd_exit(b)
        return Q

    def bwd_begin(self, Q, Bb, want_wgrad):
        """The pass's accumulators: BatchNorm sums and, with want_wgrad, the flat parameter-gradient buffer."""
        b = _BwdCursor(Q, Bb, self.groups if Bb == self.B else 1)
        Q.grad_views, Q.sums_b = self.grad_views, self.stat_sums(torch.float64)
        if not want_wgrad:
            return b
        Q.grad_flat = torch.zeros(sum(t.numel() for _, t in self.pspec), dtype=torch.float32, device=self.dev)
        if self.dt_e == L.ESR_F16:
            Q.tapmajor = E.TapMajorGrads(Q.grad_flat)
        ptr, off = {}, 0
        for name, t in self.pspec:
            ptr[name] = Q.grad_flat.data_ptr() + 4 * off
            b.poff[name] = off
            off += t.numel()
        for name in ptr:
            base = name.rsplit('.', 1)[0]
            b.params_grad.setdefault(base, (ptr.get(base + '.weight'), ptr.get(base + '.bias')))
        return b

    def before(self, li):
        """(the layer in front of recs[li] in execution order, the residual tags saved in between)"""
        k, tags = li - 1, []
        while k >= 0 and isinstance(self.recs[k], SaveRec):
            tags.append(self.recs[k].tag)
            k -= 1
        return (self.recs[k] if k >= 0 else None), tags

    def bwd_entry(self, b):
        Q, f32 = b.Q, dict(dtype=torch.float32, device=self.dev)
        if self.head is None:
            Q.gy_tensor = gin = torch.empty(b.Bb, self.ch, self.h, self.w, **f32)
        else:
            gin = self.bwd_head(b, f32)
        b.gcur = self.buf(Q, b.Bb, self.ch, self.h, self.w)
        E.layout_op(Q.bwd, self.dt_e, b.Bb, b.gcur, self.ch, 1, nchw=gin.data_ptr())

    def bwd_head(self, b, f32):
        """Backward of the linear head; returns the gradient w.r.t. the flattened features."""
        Q, Bb, bk, head, (I1, O1, O2) = b.Q, b.Bb, b.Q.bwd, self.head, self.lin_dims
        F_, H1 = self.F_.data_ptr(), self.H1.data_ptr()
        Q.gy_tensor = torch.empty(Bb, O2, **f32)
        gH1, gF = torch.empty(Bb, O1, **f32), torch.empty(Bb, I1, **f32)
        Q.keep += [gH1, gF]
        gy, w1, w2 = Q.gy_tensor.data_ptr(), head['w1'].data_ptr(), head['w2'].data_ptr()
        g2, g1 = b.params_grad.get('head2'), b.params_grad.get('head1')
        if g2 is not None:
            bk.add(L.OP_LINEAR, 'linear', _lin(2, Bb, O1, O2, L.ACT_NONE, x=H1, g=gy, dw=g2[0], db=g2[1], w=w2))
        bk.add(L.OP_LINEAR, 'linear', _lin(1, Bb, O1, O2, L.ACT_NONE, g=gy, w=w2, gx=gH1.data_ptr()))
        if g1 is not None:
            bk.add(L.OP_LINEAR, 'linear', _lin(2, Bb, I1, O1, L.ACT_LRELU, x=F_, g=gH1.data_ptr(), ysaved=H1,
                                               dw=g1[0], db=g1[1], w=w1))
        # a last conv that feeds the head through its activation without a norm layer (Discriminator_VGG_128_SN):
        # the head's input gradient is masked by that activation here (F_ holds the activation's output)
        act_last = _epilogue_act(self.recs[-1])
        o = _lin(1, Bb, I1, O1, L.ACT_LRELU, g=gH1.data_ptr(), ysaved=H1, w=w1, gx=gF.data_ptr())
        if act_last != L.ACT_NONE:
            o.x, o.in_act, b.masked = F_, act_last, True
        bk.add(L.OP_LINEAR, 'linear', o)
        return gF

    def bwd_shuffle(self, b, li):
        r = self.recs[li]
        prev, tags = self.before(li)
        if tags:
            raise L.HipExtensionError('a residual source right in front of a pixel shuffle is not supported')
        gx = self.buf(b.Q, b.Bb, 4 * r.ch, r.h, r.w)
        pl = L.esr_pool()
        pl.dtype, pl.mode, pl.B, pl.C, pl.H, pl.W = self.dt_e, L.POOL_UNSHUFFLE, b.Bb, r.ch, r.h, r.w
        pl.x, pl.g, pl.gx = r.x.view(0, 4 * r.ch), b.gcur.view(0, r.ch), gx.view(0, 4 * r.ch)
        act_prev = _epilogue_act(prev)
        if act_prev not in (L.ACT_NONE, L.ACT_RELU):
            raise L.HipExtensionError('pixel shuffle behind a LeakyReLU conv: only ReLU / no activation')
        pl.relu_mask = 1 if act_prev == L.ACT_RELU else 0
        b.Q.bwd.add(L.OP_POOL, 'pool', pl)
        b.gcur, b.masked = gx, bool(pl.relu_mask)

    def bwd_pool(self, b, li):
        r = self.recs[li]
        # sized as the pooled map's producer (odd maps: the row / column the pool drops get gradient 0, which
        # the backward leaves untouched in this zeroed buffer; its geometry is the one the conv before reads)
        gx = self.buf(b.Q, b.Bb, r.ch, r.x.H, r.x.W)
        pl = L.esr_pool()
        pl.dtype, pl.mode, pl.B, pl.C, pl.H, pl.W = self.dt_e, 1, b.Bb, r.ch, r.h, r.w
        pl.x, pl.y, pl.g, pl.gx = r.x.view(0, r.ch), r.y.view(0, r.ch), b.gcur.view(0, r.ch), gx.view(0, r.ch)
        pl.relu_mask = 1 if _epilogue_act(self.before(li)[0]) == L.ACT_RELU else 0
        b.Q.bwd.add(L.OP_POOL, 'pool', pl)
        b.gcur, b.masked = gx, bool(pl.relu_mask)

    def bwd_conv(self, b, li):
        r = self.recs[li]
        if r.res is not None:
            b.skips.setdefault(r.res, []).append(b.gcur)       # d(out)/d(saved) = 1: the skip carries gcur as it is
        if r.bn is None and r.act != L.ACT_NONE and not b.masked:
            raise RuntimeError('internal: activation mask of %s not applied' % r.key)
        gpre = b.gcur if r.bn is None else self.bn_backward(b, r)
        self.weight_grad(b, r, gpre)
        self.input_grad(b, li, gpre)

    def bn_backward(self, b, r):
        """BatchNorm backward of conv record r; returns the gradient w.r.t. the conv's output."""
        bk, gconv = b.Q.bwd, self.buf(b.Q, b.Bb, _pad32(r.cout), r.h, r.w)
        bk.add(L.OP_BN, 'bn', self.bn_op(r, L.BN_BWD_REDUCE, b, g=b.gcur))
        gbn = b.params_grad.get('bn%d' % r.ibn)
        if gbn is not None and not fuse_bn():
            o = self.bn_op(r, L.BN_BWD_FINAL, b)
            o.dgamma, o.dbeta = gbn
            bk.add(L.OP_BN, 'bn', o)
        o = self.bn_op(r, L.BN_BWD_APPLY, b, g=b.gcur, gx=gconv)
        if gbn is not None and fuse_bn():
            o.dgamma, o.dbeta = gbn          # BWD_FINAL folded into the apply pass
        bk.add(L.OP_BN, 'bn', o)
        return gconv

    def weight_grad(self, b, r, gpre):
        gw = b.params_grad.get(r.key)
        if gw is None:
            return
        wg = L.esr_wgrad()
        wg.dtype, wg.ks, wg.stride, wg.upsample = self.dt_e, r.ks, r.st, 1 if r.ups else 0
        wg.B, wg.H, wg.W, wg.cout, wg.cin = b.Bb, r.h, r.w, r.cout, r.cin
        wg.g, wg.in_ = gpre.view(0, r.cout), r.x.view(0, r.cin)
        wg.dw, wg.dbias, wg.scale = gw[0], gw[1], r.alpha
        if b.Q.tapmajor is not None and r.ks in (3, 4):
            wg.dw, wg.tap_major = b.Q.tapmajor.slot(b.poff[r.key + '.weight'], r.cout, r.cin, r.ks ** 2), 1
        # every layer owns its gradient buffers, so the weight gradient can run on the side stream
        # next to the dgrad chain (joined before the unpermute / at the end of the plan)
        # (no waits between these runs, several in flight: ESR_OPF_SIDE_FREE; each gets its own partial region)
        b.Q.bwd.add(L.OP_WGRAD, 'wgrad', wg, flags=L.OPF_SIDE | L.OPF_SIDE_FREE)

    def input_grad(self, b, li, gpre):
        r, cpg, de = self.recs[li], self.cpg, self.dp.entries
        prev, tags = self.before(li)
        resid = [g_ for t_ in tags for g_ in b.skips.get(t_, [])]
        if len(resid) > 2:
            raise L.HipExtensionError('more than two skip connections end at the input of %s' % r.key)
        gx = self.buf(b.Q, b.Bb, ((r.cin + cpg - 1) // cpg) * cpg, r.hin, r.win)
        # adjoint of (nearest x2 + 3x3 conv): a 4x4 / stride-2 conv over the gradient (esr_pack.ups_dgrad operand);
        # of a 4x4 / stride-2 conv: a 4x4 conv over the gradient spread out x2
        kw = dict(ks=4, stride=2) if r.ups else ({} if r.st == 1 else dict(ks=4, stride=1, upsample=2))
        c = E._conv(self.dt_e, b.Bb, r.hin, r.win, gpre.view(0), r.cout, None, de[r.key], L.ACT_NONE, **kw)
        c.bias = None
        act_prev = _epilogue_act(prev)
        if r.st == 2 and r.ks == 4 and act_prev == L.ACT_NONE and r.w <= 4:
            # the transposed conv of the DEEPEST stride-2 layer (8x8 output): packed tiles + split K (esr_conv.ksplit),
            # K = forward couts.  Only there: the fp32 slabs of the split grow with the OUTPUT map, and on the 16^2 /
            # 32^2 outputs their write + read (67 MB per launch) costs more than the split saves (measured:
            # 57 -> 102 us and 33 -> 100 us; profiles/r04_experiments.md)
            self.ksplit(c, b.Q.keep, b.Bb, r, transposed=True)
        c.alpha = r.alpha                                 # (backward epilogue: v = acc * alpha [+ res1] [+ res2])
        if resid:
            c.res1 = resid[0].view(0, r.cin)
            if len(resid) > 1:
                c.res2, c.beta = resid[1].view(0, r.cin), 1.0
        if act_prev != L.ACT_NONE:
            c.mask, c.out2, c.mask_cb_begin, c.mask_act = prev.y.view(0, r.cin), gx.view(0, r.cin), 0, act_prev
        else:
            c.out = gx.view(0, r.cin)
        b.Q.bwd.add_conv(c)
        b.gcur, b.masked = gx, act_prev != L.ACT_NONE

    def bwd_exit(self, b):
        Q, cin0 = b.Q, self.spec[0]['cin']
        up = Q.tapmajor.op() if Q.tapmajor is not None else None
        if up is not None:
            Q.bwd.add(L.OP_UNPERMUTE, 'unpermute', up)
        Q.gx_tensor = torch.empty(b.Bb, cin0, self.H, self.W, dtype=torch.float32, device=self.dev)
        Q.gx_op = E.layout_op(Q.bwd, self.dt_e, b.Bb, b.gcur, cin0, 0, nchw=Q.gx_tensor.data_ptr(),
                              affine=self.input_affine)
        Q.has_bn = self.nbn > 0
        Q.wgrad_arena = E.attach_wgrad_arena(Q.bwd, self.dev, exclusive=True)

    def restat(self):
        """What a SECOND forward call over the same batch (same weights) adds to the BatchNorm buffers: the groups'
        momentum updates in reverse order (the reference's netD(real), netD(fake) after netD(fake), netD(real))"""
        ops = L.OpList()
        for r in self.bn_recs:
            ops.add(L.OP_BN, 'bn', self.bn_op(r, L.BN_RESTAT))
        return ops


def build_seq_plan(spec, wp, dp, pspec, want_wgrad, B, H, W, dtype, dev, training, need_bwd,
                   input_affine=None, head=None, groups=1, bwd_B=None, dual=None):
    """dual (None | images): ONE forward whose saved activations serve TWO backward passes with their own scratch
    buffers — P (full batch, parameter gradients: the D step) and P.second (the first `dual` images only, input
    gradient only: the G step's pass through the frozen discriminator) — plus P.restat, the launch list that applies
    the BatchNorm running-statistics updates of a second forward call over the same batch in reverse group order
    (SRRaGAN_model.py:133-134 then 150-151: netD sees fake, real, then real, fake with unchanged weights, i.e. the
    same activations twice).
    groups: BatchNorm statistics groups of the batch (``forward_pair``: two reference forward calls as one
    pass; esr_bn.groups).  bwd_B: the backward covers only the first ``bwd_B`` images (the second half of a pair
    that is detached: its saved activations are the batch suffix of every buffer, so the backward launches simply
    run on the prefix) — with groups == 2 that prefix is statistics group 0.

       spec: list of dicts, in execution order:
         {'conv': key, 'cin', 'cout', 'ks', 'stride', 'act': ACT_*, 'bn': None | dict(weight,bias,rm,rv)}
             optional (round 5, SRResNet: architecture.py:13-44, block.py:199-232,299-322 as ONE launch plan):
             'ups': True        nearest x2 up-sampling folded into the conv's load (upconv_blcok)
             'res': tag, 'alpha': a    out = conv(x) * a + saved[tag]   (ResNetBlock / ShortcutBlock adds, in the epilogue)
         {'save': tag}          the current tensor is a residual source (no launch)
         {'shuffle': 2}         nn.PixelShuffle(2) (its ReLU rides in the producing conv's epilogue: it commutes)
         {'pool': True}
       head: None | dict(w1,b1,w2,b2) — flatten + Linear(.,100) + LeakyReLU + Linear(100,1)
       pspec: [(name, tensor)] in autograd-argument order; names '<convkey>.weight|bias',
       'bn<k>.weight|bias', 'head1|head2.weight|bias'.  want_wgrad: emit parameter-gradient launches.
    """
    Bb0 = B if bwd_B is None else bwd_B
    assert B % groups == 0 and (Bb0 == B or (groups > 1 and Bb0 == B // groups) or groups == 1)
    sb = SeqBuilder(spec, wp, dp, pspec, B, H, W, dtype, dev, training, input_affine, head, groups)
    sb.forward_input()
    sb.forward_layers()
    sb.forward_exit()
    P = sb.plan
    if need_bwd:
        sb.backward(P, Bb0, want_wgrad)
        if dual is not None:
            # the G step's pass: input gradient of the first `dual` images, parameters frozen
            P.second = sb.backward(BwdPass(), dual, False)
            P.restat = sb.restat()
    return P


# G32 views of each launch kind that a half of the batch advances (split_forward_groups)
_G32_FIELDS = {L.OP_CONV: ('conv', ('in_', 'out', 'aux_out', 'res1', 'res2', 'z1', 'z2', 'z3', 'mask', 'out2', 'out3')),
               L.OP_BN: ('bn', ('x', 'y', 'g', 'gx')), L.OP_POOL: ('pool', ('x', 'y', 'g', 'gx')),
               L.OP_LAYOUT: ('layout', ('g32',))}


def split_forward_groups(P, n):
    """The forward launch list of a two-group pair plan (batch 2n, BatchNorm groups (0, 1)) as TWO lists over the halves,
    so that the half whose input is known early (the train step's ``real`` operand, group 1) can run long before the
    other one exists (round 5: netD(real) under the generator's forward instead of behind it).  Every launch of the
    full list is copied with B = n, its buffers advanced to the half's images, BatchNorm launches with groups = 1 and
    the statistics arrays advanced to the group's [C] rows.  The reference's order of running-statistics updates is
    (group 0, group 1): the EARLY half (group 1) therefore leaves the running buffers alone and the update it owes is a
    third list, ``P.restat1`` (ESR_BN_RESTAT on group 1's sums), to be run once after the late half.
    Returns nothing; fills P.fwd_half = [list of group 0, list of group 1] and P.restat1."""
    src = P.fwd.array()
    halves = [L.OpList(), L.OpList()]
    restat1 = L.OpList()
    for g in (0, 1):
        for i in range(len(P.fwd.ops)):
            o = L.esr_op.from_buffer_copy(src[i])
            k = o.kind
            if k in _G32_FIELDS:
                st = getattr(o.u, _G32_FIELDS[k][0])
                for fld in _G32_FIELDS[k][1]:
                    v = getattr(st, fld)
                    if v.ptr:
                        v.ptr = v.ptr + g * n * v.batch_stride
                assert st.B == 2 * n, 'pair plan: every launch covers both halves'
                st.B = n
                if k == L.OP_CONV:
                    if st.nchw_out:
                        raise L.HipExtensionError('split pair forward: NCHW conv outputs are not supported')
                    if st.stat_sums:
                        assert st.stat_groups == 2
                        st.stat_sums = st.stat_sums + g * 2 * st.stat_C * 8
                        st.stat_groups = 1
                elif k == L.OP_BN:
                    assert st.groups == 2
                    st.groups = 1
                    st.sums = st.sums + g * 2 * st.C * 8
                    st.mean = st.mean + g * st.C * 4
                    st.invstd = st.invstd + g * st.C * 4
                    if g == 1:
                        st.running_mean = st.running_var = st.num_batches_tracked = None
                elif k == L.OP_LAYOUT:
                    if st.nchw and i != P.in_op:
                        st.nchw = st.nchw + g * n * st.C * st.H * st.W * 4
            elif k == L.OP_LINEAR:
                st = o.u.linear
                assert st.B == 2 * n and st.mode == 0
                st.B = n
                st.x = st.x + g * n * st.I * 4
                st.y = st.y + g * n * st.O * 4
            else:
                raise L.HipExtensionError('split pair forward: launch kind %d is not supported' % k)
            halves[g].ops.append(o)
    for i in range(len(P.restat.ops)):
        o = L.esr_op.from_buffer_copy(P.restat.array()[i])
        st = o.u.bn
        assert o.kind == L.OP_BN and st.groups == 2 and st.B == 2 * n
        st.B, st.groups = n, 1
        st.sums = st.sums + 2 * st.C * 8
        restat1.ops.append(o)
    P.fwd_half, P.restat1 = halves, restat1


def group0_restat(P, n):
    """The launch list (built once, kept in ``P.restat0``) that gives the BatchNorm buffers of a two-group dual plan
    (batch 2n) the momentum update of ONE more forward call over group 0 with unchanged weights — the standard-GAN step's
    third netD call (SRGAN_model.py:129, 140, 143: fake, real, fake; the forward did the first two).  Copies of
    ``P.restat``'s launches as ``split_forward_groups`` makes ``restat1``, on group 0: B = n, groups = 1, the sums left
    at group 0's rows; ``num_batches_tracked`` goes up by one per layer."""
    if P.restat0 is None:
        ops = L.OpList()
        for i in range(len(P.restat.ops)):
            o = L.esr_op.from_buffer_copy(P.restat.array()[i])
            st = o.u.bn
            assert o.kind == L.OP_BN and st.groups == 2 and st.B == 2 * n
            st.B, st.groups = n, 1
            ops.ops.append(o)
        P.restat0 = ops
    return P.restat0


def _begin_pass(Q, gx_ptr, accumulate):
    """Zero what the pass Q accumulates into and bind the layout op that exports its input gradient (gx_ptr None: a
    captured graph replays the list, with the build-time binding baked in)."""
    if Q.has_bn:
        Q.sums_b.zero_()
    if Q.grad_flat is not None:
        Q.grad_flat.zero_()
        if Q.tapmajor is not None:
            Q.tapmajor.tm.zero_()
    if gx_ptr is not None:
        lo = Q.bwd.array()[Q.gx_op].u.layout
        lo.nchw, lo.accumulate = gx_ptr, accumulate


def _run_pass(Q, graph, gy, n_total, want_gx, needs):
    """Replay one backward pass (a SeqPlan's own or its BwdPass) for the upstream gradient gy; returns
    (gx or None, [parameter gradients or None])."""
    st = E.current_stream()
    nb_ = Q.gy_tensor.shape[0]              # images the pass covers (a pair's first half, or all)
    Q.gy_tensor.copy_(gy.detach()[:nb_].reshape(Q.gy_tensor.shape))
    _begin_pass(Q, None if graph else Q.gx_tensor.data_ptr(), 0)
    if graph:
        Q.bwd.graph_launch(st)
    else:
        Q.bwd.run(st)
    gx = None
    if want_gx:
        gx = Q.gx_tensor.clone()
        if nb_ < n_total:                    # detached second half: zero gradient
            gx = torch.cat([gx, gx.new_zeros((n_total - nb_,) + tuple(gx.shape[1:]))])
    grads = [None] * len(needs)
    if Q.grad_flat is not None:
        flat = Q.grad_flat.clone()
        off = 0
        for i, (numel, shape) in enumerate(Q.grad_views):
            if needs[i]:
                grads[i] = flat[off:off + numel].view(shape)
            off += numel
    return gx, grads


def run_pass_into(Q, gx_into=None, accumulate=False):
    """The hand-written train step's face of a backward pass: the upstream gradient is ALREADY in Q.gy_tensor (the loss
    kernel wrote it there), the input gradient goes to ``gx_into`` (NCHW fp32; ``accumulate``: added to what it holds)
    or is dropped into the pass's own buffer, the parameter gradients stay in Q.grad_flat (OIHW order of the plan's
    parameter list).  No copies, no clones."""
    _begin_pass(Q, (gx_into if gx_into is not None else Q.gx_tensor).data_ptr(),
                1 if (accumulate and gx_into is not None) else 0)
    Q.bwd.run(E.current_stream())


def bind_param_grads(Q, mod):
    """Points the `.grad` of `mod`'s parameters at views of Q.grad_flat (made once; pspec order): what run_pass_into left
    there is what an optimizer reads, in place."""
    if Q.param_views is None:
        views, off = [], 0
        for numel, shape in Q.grad_views:
            views.append(Q.grad_flat[off:off + numel].view(shape))
            off += numel
        Q.param_views = views
        Q.param_list = [t for _, t in mod._pspec()]
    for p, v in zip(Q.param_list, Q.param_views):
        p.grad = v


class SeqNetFn(torch.autograd.Function):
    """One autograd node for a whole feed-forward plan."""

    @staticmethod
    def forward(ctx, x, mod, *params):
        out, lease = mod._run_forward(x, need_bwd=True, **getattr(mod, '_pair_opts', {}))
        ctx.mod, ctx.lease, ctx.n = mod, lease, len(params)
        return out

    @staticmethod
    def backward(ctx, gy):
        P = ctx.lease.plan
        if P is None:
            raise RuntimeError('backward called twice on the same forward (retain_graph unsupported)')
        gx, grads = _run_pass(P, P.graph, gy, gy.shape[0], ctx.needs_input_grad[0], ctx.needs_input_grad[2:])
        ctx.lease.release()
        return (gx, None) + tuple(grads)


class SharedPass:
    """Handle of ONE forward over [a; b] whose activations serve two backward passes (build_seq_plan(dual=...)):
    the pass that gave `a` its gradient (first_fn) and `second_pass()`, which re-issues the same outputs attached to
    the module's parameters — what a second pair of forward calls with unchanged weights would compute
    (SRRaGAN_model.py:150-151 after 133-134) — and applies that second pair's BatchNorm buffer updates."""

    def __init__(self, mod, lease, out, n):
        self.mod, self.lease, self.out, self.n = mod, lease, out, n
        self.pending = 2

    def done(self):
        self.pending -= 1
        if self.pending <= 0 and self.lease is not None:
            self.lease.release()
            self.lease = None

    def second_pass(self):
        """(pred_b, pred_a): the second pair in the reference's order (real first), differentiable w.r.t. the module's
        parameters only."""
        if self.lease is None or self.lease.plan is None:
            raise RuntimeError('SharedPass.second_pass: the forward\'s activations were released')
        y = SharedSecondFn.apply(self, *[t for _, t in self.mod._pspec()])
        return y[self.n:], y[:self.n]

    def __del__(self):
        if self.lease is not None:
            self.lease.release()


class SharedFirstFn(torch.autograd.Function):
    """netD over [a; b] in one pass (BatchNorm statistics per half); backward: input gradient of `a` only."""

    @staticmethod
    def forward(ctx, a, b, mod, holder):
        n = a.shape[0]
        x = torch.cat([a.detach(), b.detach()])
        out, lease = mod._run_forward(x, need_bwd=True, groups=2 if mod._has_bn else 1, dual=n)
        h = SharedPass(mod, lease, out, n)
        holder.append(h)
        ctx.h = h
        return out

    @staticmethod
    def backward(ctx, gy):
        h = ctx.h
        if h is None or h.lease is None or h.lease.plan is None:
            raise RuntimeError('backward called twice on the same forward (retain_graph unsupported)')
        P = h.lease.plan
        gx, _ = _run_pass(P.second, False, gy, h.n, True, ())
        ctx.h = None
        h.done()
        return gx, None, None, None


class SharedSecondFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, *params):
        P = h.lease.plan
        if P.restat is not None and P.restat.ops:
            P.restat.run(E.current_stream())
        ctx.h, ctx.n = h, len(params)
        return h.out.clone()

    @staticmethod
    def backward(ctx, gy):
        h = ctx.h
        if h is None or h.lease is None or h.lease.plan is None:
            raise RuntimeError('backward called twice on the same forward (retain_graph unsupported)')
        P = h.lease.plan
        _, grads = _run_pass(P, False, gy, gy.shape[0], False, ctx.needs_input_grad[1:])
        ctx.h = None
        h.done()
        return (None,) + tuple(grads)
