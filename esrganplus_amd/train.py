"""ESRGAN+ training step on the HIP path — the call pattern of
``SRRaGANModel.optimize_parameters`` (codes/models/SRRaGAN_model.py:113-186) with the
hyper-parameters of codes/options/train/train_ESRGANplus.json:55-77: L1 pixel x0.01, L1 VGG-feature
x1, relativistic-average GAN (BCE-with-logits) x0.005, Adam(1e-4, betas (0.9, 0.999)) for G and D.

The three networks are the drop-in HIP modules; the losses are a handful of tiny reductions.  With
``torch.distributed`` initialised (one process per GPU) the step is data-parallel: gradient
exchanges are started right after each backward and waited for right before the matching
``optimizer.step()``, so the G exchange overlaps the whole D forward/backward (the D step only uses
``fake_H.detach()`` computed before the G update, exactly as in the reference).

Launch economy (the step is a few thousand small launches): each network sees its two operands in ONE pass
(``forward_pair``: per-operand BatchNorm statistics), the losses are single launches that also produce their
gradients (``losses``), and the D step is enqueued on a second stream under the G backward (one GPU and
data-parallel alike: the step that is measured on one GPU is the step that scales).

Three steps share one base (``_StepBase``) and, in their hand-written form, one set of phases (``_ManualPass`` and
what derives from it; DESIGN.md 7 has the table of streams, waits and records): ``ESRGANPlusStep``, ``PSNRStep`` (the
generator-only subset) and ``SRGANStep``.
"""
import contextlib
import os

import torch

from . import convnet as CN
from . import dp as DP
from . import engine as E
from . import functional as Fn
from . import losses as LS
from .optim import FusedAdam, DynamicLossScaler

# the step's log (SRRaGAN_model.py:171-186), in the order the logging form copies it to the host
LOG_KEYS = ('l_g_pix', 'l_g_fea', 'l_g_gan', 'l_d_real', 'l_d_fake', 'D_real', 'D_fake')


def _log_values(l_g_pix, l_g_fea, l_g_gan, aux):
    return (l_g_pix, l_g_fea, l_g_gan, aux[2], aux[3], aux[0], aux[1])          # LOG_KEYS order


def _buffer_like(buf, ref):
    """`buf` when it has `ref`'s shape and device, else a new (uninitialised) tensor like `ref`."""
    if buf is None or buf.shape != ref.shape or buf.device != ref.device:
        buf = torch.empty_like(ref)
    return buf


def _validate(self, lr_images, hr_images, x8=False, **tiling):
    """The validation pass of codes/train.py:121-159 on one image set: ``finish()``, then the generator's
    ``evaluate_images(lr_images, hr_images, **tiling)`` — always the eval forward, the module's mode left as it is — ->
    the average RGB PSNR as a float (train.py:148-150; cropped by the scale).  ``x8=True`` scores the x8 self-ensemble
    (``evaluate_images(x8=True)``, the reference's ``test_x8``).  The per-image table (psnr, ssim, psnr_y, ssim_y) stays
    on ``self.val_result``.  Valid between pipelined steps, as ``test()`` is; the read-back of the table is the one
    synchronisation."""
    self.finish()
    if not hasattr(self.netG, 'evaluate_images'):
        raise ValueError('validate needs a generator with evaluate_images (RRDBNet / RRDB_Net at x4), got %s'
                         % type(self.netG).__name__)
    if x8:
        tiling['x8'] = True
    self.val_result = self.netG.evaluate_images(lr_images, hr_images, **tiling)[1]
    return self.val_result.averages()[0]


def _validate_hr(self, hr_images, **tiling):
    """``validate`` from ground-truth images alone (the reference's ``dataroot_LR: null``): ``finish()``, then the
    generator's ``evaluate_hr_images(hr_images, **tiling)`` -> the average RGB PSNR as a float; the per-image table stays
    on ``self.val_result``.  Valid between pipelined steps, as ``validate`` is.  Not offered: ``x8``."""
    self.finish()
    if not hasattr(self.netG, 'evaluate_hr_images'):
        raise ValueError('validate_hr needs a generator with evaluate_hr_images (RRDBNet / RRDB_Net at x4), got %s'
                         % type(self.netG).__name__)
    self.val_result = self.netG.evaluate_hr_images(hr_images, **tiling)[1]
    return self.val_result.averages()[0]


def _check_channels(what, netG, netD, netF):
    """The generator's images are what the discriminator and the feature extractor read: their channel counts must
    agree before a step is built (the networks' plans take the first conv's channels on trust from their caller)."""
    g = getattr(getattr(netG, 'module', netG), 'out_nc', None)
    d = getattr(getattr(netD, 'module', netD), 'in_nc', None)
    if g is None:
        return
    if d is not None and g != d:
        raise ValueError('%s: netD expects %d input channels (in_nc), got a generator with out_nc = %d' % (what, d, g))
    if netF is not None and g != 3:
        raise ValueError('%s: the feature term (VGG) expects 3 input channels, got a generator with out_nc = %d; '
                         'train such a generator without it (SRGANStep with feature_weight = 0, or PSNRStep)' % (what, g))


class _StepBase:
    """What the three steps share: the loss scale, the optimizer / exchange pair of each network that trains, the
    stream and knob helpers, and the public calls that do not depend on the losses."""

    _nets = ('G', 'D')            # the networks this step trains: net<X>, optimizer_<X>, ex<X>

    def __init__(self, netG, loss_scale, data_parallel):
        self.netG = netG
        # data_parallel: None = follow torch.distributed (world size > 1); False inside a multi-rank job = this rank's
        # own step without any exchange (bench.py's no-exchange figure next to the data-parallel one)
        self.data_parallel = DP.active() if data_parallel is None else bool(data_parallel)
        # fp16 path: 'dynamic' (default policy of the scaler: start at 1024, halve on overflow and skip that step,
        # double after 2000 clean steps) or a fixed number (1.0 for fp32).  Nothing here synchronises with the host.
        self.scaler = None
        if loss_scale == 'dynamic':
            self.scaler = DynamicLossScaler(next(netG.parameters()).device)
            loss_scale = 1.0
        self.loss_scale = loss_scale
        self.log = {}
        self.fake_H = None
        self._steps = 0
        # what the hand-written step keeps between calls: the buffers dL/d fake_H is collected in, the pinned host copy
        # of the log, the event behind the tail a step left on the side stream; the static loss scale as a device scalar
        # (autograd form); `_marks`: a list set from outside (tools/train_marks.py) collects (name, timed event) pairs
        self._gy = self._gy2 = self._log_host = self._ev_tail = None
        self._scale_tensor = self._scale_value = None
        self._marks = None
        # stream overlap of the step (ESR_TRAIN_OVERLAP): 0 = everything in sequence on the caller's stream (9.8 ms);
        # 1 (default) = netF(var_H) and the D step on a second stream (8.9 ms).  Measured, round 4
        # (profiles/r04_experiments.md): more concurrency is NOT faster here — the G step's netD pass on a third stream
        # next to its netF pass costs 0.1-0.15 ms over 1, streams probed to be truly concurrent 0.4-0.9 ms,
        # GPU_MAX_HW_QUEUES=8 3-5 ms: a persistent chain launch (128 lock-stepped workgroups exchanging halos) that
        # shares the chip with other launches runs at the pace of its most-delayed tile, and the small launches slow
        # each other 2-5x.  What mode 1 overlaps is what the default stream's hardware queue lets through.
        self.overlap = self._knob_int('ESR_TRAIN_OVERLAP', '1', (0, 1))
        # ESR_TRAIN_MANUAL=0: the step is written with autograd (losses as autograd Functions, torch.autograd.backward
        # over the networks' nodes: ~100 glue launches — clones, gradient copies / sums, zero fills — and their
        # host time per step).  Default: the same launch lists driven directly (`_step_manual`), when the networks
        # allow it (`_manual_ok`)
        self.manual = os.environ.get('ESR_TRAIN_MANUAL', '1') != '0'

    def _optimizer(self, net, params, lr, beta1, weight_decay=0.0):
        """One fused launch per optimizer (optim.FusedAdam == torch.optim.Adam arithmetic; it stays a
        torch.optim.Optimizer, so the reference's MultiStepLR schedulers attach unchanged) and the network's gradient
        exchange -> (optimizer, exchange)."""
        return (FusedAdam(params, lr=lr, betas=(beta1, 0.999), weight_decay=weight_decay),
                DP.GradExchange(net, enabled=self.data_parallel, measure=self.data_parallel))

    @staticmethod
    def _knob(name, default, allowed):
        v = os.environ.get(name, default)
        if v not in allowed:          # (a misspelt ESR_TRAIN_DSTEP used to mean: the D step never runs)
            raise ValueError('%s=%r: expected one of %s' % (name, v, ', '.join(allowed)))
        return v

    @classmethod
    def _knob_int(cls, name, default, allowed):
        return int(cls._knob(name, default, tuple(str(a) for a in allowed)))

    def _side(self, dev):
        # a plain new stream (cached), which measured faster than one probed to run concurrently (see `overlap` above)
        return E.concurrent_streams(dev, 1)[0]

    def _scale_t(self, dev):
        t = self._scale_tensor
        if t is None or t.device != dev or float(self._scale_value) != float(self.loss_scale):
            t = self._scale_tensor = torch.full((), float(self.loss_scale), dtype=torch.float32, device=dev)
            self._scale_value = float(self.loss_scale)
        return t

    def _scale(self, dev):
        """The loss scale the autograd forms multiply into their backward: the scaler's device scalar, or the static one."""
        return self.scaler.scale if self.scaler else self._scale_t(dev)

    def _zero_stale_grads(self):
        netG = self.netG
        if not (hasattr(netG, 'mark_grads_stale') and netG.mark_grads_stale()):
            self.optimizer_G.zero_grad(set_to_none=True)     # (first step / gradients that are not the module's store)

    def _grad_buffer(self, fake):
        """The buffer dL/d fake_H is collected in (uninitialised: the pixel loss, or the first pass into it, writes it)."""
        self._gy = _buffer_like(self._gy, fake)
        return self._gy

    def _generator(self, var_L, z):
        return self.netG(var_L, z=z) if z is not None else self.netG(var_L)

    def _trained(self, what):
        return [getattr(self, what + t) for t in self._nets]

    # ---- exchange accounting (bench.py dp_train) ----
    def comm_reset(self):
        self._steps = 0
        for ex in self._trained('ex'):
            ex.reset_counters()

    def comm_report(self):
        """Per step: all-reduce calls / bytes of the step's gradient exchanges and the milliseconds the compute streams
        spent blocked on them (HIP events around the waits); with two exchanges, the latter for each as well.
        Synchronises the device."""
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        n = max(self._steps, 1)
        exs = self._trained('ex')
        rep = {'calls_per_step': sum(ex.calls for ex in exs) / n,
               'bytes_per_step': sum(ex.bytes for ex in exs) / n,
               'exposed_ms_per_step': sum(ex.exposed_ms() for ex in exs) / n}
        if len(exs) > 1:
            rep.update(('exposed_ms_per_step_' + t, ex.exposed_ms() / n) for t, ex in zip(self._nets, exs))
        return rep

    def _defer_networks(self, ev):
        # the networks' PUBLIC entry points (forward / forward_pair / state_dict) order this event in front of their
        # caller's stream (block._PlannedModule._join_pending): a validation forward or a checkpoint between two steps
        # sees the finished optimizer updates and weight packs without the loop having to call finish()
        for net in self._trained('net'):
            if hasattr(net, '_defer_to'):
                net._defer_to(ev)

    def state_dict(self):
        """The optimizers' states (base_model.py:65-74 `save_training_state`), ordered behind whatever a pipelined
        step left in flight."""
        self.finish()
        return {'optimizers': [o.state_dict() for o in self._trained('optimizer_')]}

    def finish(self):
        """Orders what a pipelined step (``step(..., sync_log=False)``) left on the side stream — the end of the D
        step, D's Adam, the weight packs — in front of the current stream: call it (or synchronise the device) before
        reading the networks' parameters, buffers or the logged losses after such a step."""
        if self._ev_tail is not None:
            torch.cuda.current_stream().wait_event(self._ev_tail)

    def test(self, var_L):
        """The reference models' ``test`` (SR_model.py:76-80, SRGAN_model.py:180-184): the eval forward without
        gradient; the generator is back in training mode afterwards.  Valid between pipelined steps (the generator's
        forward joins what they left in flight)."""
        E.require_cuda(var_L, '%s.test: var_L' % type(self).__name__)
        self.netG.eval()
        try:
            with torch.no_grad():
                self.fake_H = self.netG(var_L)
        finally:
            self.netG.train()
        return self.fake_H


class _ManualPass:
    """One call of a `_step_manual`: what its phases hand to each other, and the phases themselves.  This class has the
    generator's own (all of `PSNRStep`'s but the tail); `_GANPass` adds netF's and netD's.  Every phase only enqueues;
    `read_log` is the one place where the host waits.  The drivers list the phases in the order in which the HOST
    enqueues them; DESIGN.md 7 lists what each waits for and records."""

    def __init__(self, st, var_L, var_H, z, sync_log):
        self.st, self.sync_log = st, sync_log
        self.var_L, self.var_H, self.z = var_L, var_H, z
        self.n = var_L.shape[0]
        self.S = float(st.loss_scale)
        self.sdev = st.scaler.state if st.scaler else None          # state[0] = the dynamic loss scale (device)
        self.main = torch.cuda.current_stream()
        self.side = st._side(var_L.device) if st.overlap >= 1 else None
        self.fake = self.stG = self.gy = self.l_g_pix = None
        self.ev0 = self.ev_prep = self.ev_log = None

    def mark(self, name):
        marks = self.st._marks          # measurement (tools/train_marks.py): timed events on the main stream
        if marks is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record(self.main)
            marks.append((name, e))

    def generator_forward(self):
        st = self.st
        if self.side is not None:
            self.ev0 = torch.cuda.Event()
            # var_H, whatever the caller did before the step, and the previous step's Adam (it read the buffer that
            # `prepare_backward` zeroes)
            self.ev0.record(self.main)
        # the generator's forward is enqueued FIRST: a loop that reads its losses every step has the host running
        # behind the GPU, and the step's critical path starts with this launch list, not with netF(real)
        self.fake, self.stG = Fn.rrdbnet_train_forward(st.netG, self.var_L, self.z)
        st.fake_H = self.fake
        self.mark('G forward')

    def prepare_backward(self):
        # the G backward's step-independent preliminaries (zero fills of the gradient buffers, the backward
        # chain's weight-stream gather) under the generator's forward instead of in front of the backward
        Fn.rrdbnet_train_prepare(self.st.netG, self.stG)
        self.ev_prep = torch.cuda.Event()
        self.ev_prep.record(self.side)

    def under_generator_forward(self):
        """What does not depend on the generator, on the side stream under its forward (behind the previous step's
        input-gradient packs, in order).  Without a side stream the backward prepares itself."""
        if self.side is None:
            return
        self.side.wait_event(self.ev0)
        with torch.cuda.stream(self.side):
            self.prepare_backward()

    def pixel_loss(self):
        # writes dL/d fake_H's buffer; a step without the term (`_pix_raw` None) leaves that to the first pass into it
        st = self.st
        self.gy = st._grad_buffer(self.fake)
        if st._pix_raw is not None:
            self.l_g_pix = st._pix_raw(self.fake, self.var_H, st.l_pix_w, grad_out=self.gy, grad_scale=self.S,
                                       scale_dev=self.sdev)

    def generator_backward(self):
        st = self.st
        if self.ev_prep is not None:
            self.main.wait_event(self.ev_prep)
        Fn.rrdbnet_train_backward(st.netG, self.stG, self.gy, follow_wgs=st.follow_wgs_sync if self.sync_log else None)
        self.mark('G backward (tail, chain, weight gradients, unpermute)')
        st.exG.start()


class _PSNRPass(_ManualPass):
    """`PSNRStep`'s own: the loss copied to the host right behind its launch, and a tail whose Adam stays on the main
    stream (with the scaler), the input-gradient packs alone behind it on the side stream."""

    def pixel_loss(self):
        super().pixel_loss()
        if self.sync_log:
            # the host reads the loss, not the end of the step: copied right behind the loss launch
            st = self.st
            if st._log_host is None:
                st._log_host = torch.empty(1, dtype=torch.float32).pin_memory()
            st._log_host.copy_(self.l_g_pix.reshape(1), non_blocking=True)
            self.ev_log = torch.cuda.Event()
            self.ev_log.record(self.main)

    def tail(self):
        st, netG, side = self.st, self.st.netG, self.side
        st.exG.wait()
        st.optimizer_G.step(grad_scale=1.0 / self.S, scaler=st.scaler)
        if st.scaler:
            st.scaler.update()
        netG.prepack(fwd=True, dgrad=False)       # what the next forward starts with
        if side is None:
            netG.prepack(fwd=False, dgrad=True)
            return
        side.wait_stream(self.main)               # G's new weights
        with torch.cuda.stream(side):
            netG.prepack(fwd=False, dgrad=True)
            st._ev_tail = torch.cuda.Event()
            st._ev_tail.record(side)
        st._defer_networks(st._ev_tail)           # netG's public entry points (forward, state_dict) join the tail

    def read_log(self):
        st = self.st
        if not self.sync_log:
            st.log = {'l_pix': self.l_g_pix}
            return st.log
        self.ev_log.synchronize()
        st.log = {'l_pix': float(st._log_host[0])}
        st.finish()                               # the default call: everything ordered on the current stream
        return st.log


class _GANPass(_ManualPass):
    """The phases of a step with a discriminator (and, unless the step has no feature term, netF) around the
    generator's.  The step's policy is read from its attributes `d_when` / `d_when_sync`, `netf_side`, `d_split` and
    `follow_wgs_sync`; what the two GAN steps compute differently is in `_ESRGANPass` / `_SRGANPass`: `g_gan_loss`,
    `d_gan_loss`, `d_restat`, `in_sequence`, `tail_on_main`, `read_log`, and `join_netd`."""

    join_netd = False             # netD._join_pending() in front of a netD forward that had no early half

    def __init__(self, st, var_L, var_H, var_ref, z, sync_log):
        super().__init__(st, var_L, var_H, z, sync_log)
        self.var_ref = var_ref
        self.has_fea = st._fea_raw is not None
        self.d_when = st.d_when_sync if sync_log else st.d_when
        self.real_fea = self.d_early = self.ev_f = None
        self.leaseF = self.PF = self.leaseD = self.PD = self.out = None
        self.l_g_fea = self.l_g_gan = self.aux = None

    def under_generator_forward(self):
        """What does not depend on the generator, on the side stream under its forward: netF(real), the G backward's
        preliminaries, the `real` half of a two-stage netD forward."""
        st, side = self.st, self.side
        if side is None:
            return
        netD = st.netD
        dsplit = (st.d_split and netD._has_bn and netD.training and not E.use_graphs()
                  and not getattr(netD, '_per_call_weights', False))
        side.wait_event(self.ev0)
        with torch.cuda.stream(side):
            if self.has_fea:
                self.real_fea = st.netF._run_forward(self.var_H, need_bwd=False)[0]
            self.prepare_backward()
            if dsplit:
                # netD(real): the previous step's D-side tail (Adam, packs) sits on this stream, in front of it
                self.var_ref.record_stream(side)
                self.d_early = netD._pair_begin(self.var_ref) + (torch.cuda.Event(),)
                self.d_early[2].record(side)
        if self.has_fea:
            self.real_fea.record_stream(self.main)

    def netf_fake(self):
        st = self.st
        fake_fea, self.leaseF = st.netF._run_forward(self.fake, need_bwd=True)
        self.PF = self.leaseF.plan
        self.l_g_fea = st._fea_raw(fake_fea, self.real_fea, st.l_fea_w, grad_out=self.PF.gy_tensor,
                                   grad_scale=self.S, scale_dev=self.sdev)

    def netd_forward(self):
        st, main, d_early = self.st, self.main, self.d_early
        netD = st.netD
        if st._ev_tail is not None:
            main.wait_event(st._ev_tail)              # the previous step's D step, D's Adam and packs (side stream)
        # ONE netD forward for all of the step's calls (forward_shared): groups (fake, real)
        if d_early is not None:
            self.PD, self.leaseD = d_early[0], d_early[1]
            main.wait_event(d_early[2])               # the real half (side stream)
            self.out = netD._pair_finish(self.PD, self.fake)
        else:
            if self.join_netd:
                netD._join_pending()
            self.out, self.leaseD = netD._run_forward(torch.cat([self.fake, self.var_ref]), need_bwd=True,
                                                      groups=2 if netD._has_bn else 1, dual=self.n)
            self.PD = self.leaseD.plan
        if self.side is not None:
            self.out.record_stream(self.side)         # (the D step reads it there)
        self.l_g_gan = self.g_gan_loss(self.out, self.PD.second.gy_tensor)

    def feature_and_gan_forward(self):
        """netF(fake) with the feature loss and netD's forward with the GAN loss, next to each other or in sequence."""
        st, main, side = self.st, self.main, self.side
        if not self.has_fea:
            self.netd_forward()
        elif st.netf_side and side is not None:
            # netF(fake) — forward, feature loss, input-gradient pass — on the side stream next to netD's forward and
            # G-step pass on the main stream.  The HOST enqueues the main stream's netD forward first (it is the longer
            # chain: the G backward hangs off it); the two input gradients meet in one add.
            st._gy2 = _buffer_like(st._gy2, self.fake)
            side.wait_stream(main)                        # fake_H (behind the pixel loss)
            self.fake.record_stream(side)
            self.netd_forward()
            with torch.cuda.stream(side):
                self.netf_fake()
                CN.run_pass_into(self.PF, gx_into=st._gy2, accumulate=False)
                self.ev_f = torch.cuda.Event()
                self.ev_f.record(side)
        else:
            if side is not None:
                main.wait_stream(side)
            else:
                self.real_fea = st.netF._run_forward(self.var_H, need_bwd=False)[0]
            self.in_sequence()
        self.mark('pixel loss, netD(fake) forward, GAN loss')

    def fork_d_step(self):
        if self.side is not None:
            # all the D step waits for, WHEREVER it is enqueued: netD's forward and the GAN loss (not the G backward)
            self.side.wait_stream(self.main)

    def d_step(self):
        # the D step (SRRaGAN_model.py:143-168, SRGAN_model.py:137-160): its calls see the first pass's values
        st, PD = self.st, self.PD
        cur = E.current_stream()
        if self.d_early is not None and PD.restat1.ops:
            PD.restat1.run(cur)                           # the running-statistics update the early half still owes
        if PD.restat is not None and PD.restat.ops:
            self.d_restat(PD).run(cur)
        self.aux = self.d_gan_loss(self.out, PD.gy_tensor)        # plan order [fake; real]
        CN.run_pass_into(PD)
        CN.bind_param_grads(PD, st.netD)
        st.exD.start()

    def place_d_step(self, pos):
        """Enqueues the D step on the side stream if `pos` ('first', 'mid', 'last': where the driver stands) is where
        this call wants it; without a side stream, once on the main stream behind the G backward ('last').  The side
        stream's wait for the D step's inputs is `fork_d_step`, in front of the 'first' position."""
        # When the host enqueues the D step (~60 launches, ~0.5-1 ms of host time during which the main stream gets
        # nothing new).  Round 4, same box, ms per step with netF(fake) on the main / side stream: 'first' (before
        # the main stream's backward passes) 8.03 / 7.92, 'mid' 8.05 / 7.92, 'last' (behind the G backward's launch:
        # it then runs under the backward chain) 8.35 / 7.57.
        # Where the HOST enqueues it matters as much: the D step is ~60 launches (~1 ms of host time) during which the
        # main stream gets nothing new.  'mid': the main stream's netD / netF input-gradient passes (two C calls,
        # ~0.9 ms of GPU work) go out first and run while the host enqueues the D step; the G backward follows.
        side = self.side
        if side is None:
            if pos == 'last':
                self.d_step()
            return
        if pos == self.d_when:
            with torch.cuda.stream(side):
                self.d_step()

    def input_gradients(self):
        # dL/d fake_H: + d l_gan (netD, first pair) + d l_fea (netF), added by the passes' last layout ops (netD's
        # WRITES the buffer when no pixel loss did)
        gy = self.gy
        CN.run_pass_into(self.PD.second, gx_into=gy, accumulate=self.l_g_pix is not None)
        self.mark('netD input-gradient pass (G step)')
        if self.ev_f is not None:
            self.main.wait_event(self.ev_f)
            gy.add_(self.st._gy2)
            self.mark('wait for netF(fake) pass, add')
        elif self.PF is not None:
            CN.run_pass_into(self.PF, gx_into=gy, accumulate=True)

    def release(self):
        if self.leaseF is not None:
            self.leaseF.release()
        self.leaseD.release()

    def tail(self):
        # The step's tail.  With a side stream and a static loss scale the main stream only carries what the NEXT
        # generator forward waits for — G's Adam and the pack of its forward weights; the D step's end, D's Adam, D's
        # packs and G's input-gradient packs stay on the side stream, and the main stream meets them again (_ev_tail)
        # in front of the next netD forward.  Else (dynamic loss scaler, or no side stream): ordered on the main stream.
        # Only in the pipelined form of the call (sync_log=False: the caller reads nothing before `finish()` / a device
        # synchronisation); the default call returns with everything ordered on the current stream (`read_log`).
        st, main, side = self.st, self.main, self.side
        if side is None or st.scaler is not None:
            if side is not None:
                main.wait_stream(side)
            self.tail_on_main()
            return
        inv = 1.0 / st.loss_scale
        st.exG.wait()
        st.optimizer_G.step(grad_scale=inv, scaler=None)
        st.netG.prepack(fwd=True, dgrad=False)
        self.mark('Adam(G), forward weight pack')
        side.wait_stream(main)                        # G's new weights (its input-gradient packs read them)
        with torch.cuda.stream(side):
            st.exD.wait()
            st.optimizer_D.step(grad_scale=inv, scaler=None)
            st.netD.prepack()
            st.netG.prepack(fwd=False, dgrad=True)
            st._ev_tail = torch.cuda.Event()
            st._ev_tail.record(side)
        st._defer_networks(st._ev_tail)


class _ESRGANPass(_GANPass):
    """`ESRGANPlusStep`'s own: the relativistic-average losses, netD's whole replay of running statistics, and the log
    gathered into pinned memory on the side stream (`gather_log` / `read_log`)."""

    def __init__(self, *args):
        super().__init__(*args)
        self.ev_glog = self.log_keep = None

    def g_gan_loss(self, out, grad_fake):
        # G step: BCE(pred_d_real - mean(pred_g_fake), 0) + BCE(pred_g_fake - mean(pred_d_real), 1), gradient to the fake half
        n, st = self.n, self.st
        return LS.ragan_raw(out[n:], out[:n], False, True, st.l_gan_w, grad_x=None, grad_y=grad_fake,
                            grad_scale=self.S, scale_dev=self.sdev, global_mean=st.data_parallel)[0]

    def d_gan_loss(self, out, gyt):
        n = self.n
        return LS.ragan_raw(out[n:], out[:n], True, False, 1.0, grad_x=gyt[n:], grad_y=gyt[:n],
                            grad_scale=self.S, scale_dev=self.sdev, global_mean=self.st.data_parallel)[1]

    def d_restat(self, PD):
        return PD.restat                  # the second pair of calls: real, fake

    def in_sequence(self):
        self.netf_fake()
        self.netd_forward()

    def feature_and_gan_forward(self):
        super().feature_and_gan_forward()
        if self.sync_log and self.side is not None:
            self.ev_glog = torch.cuda.Event()         # the G step's three losses are enqueued (main; l_g_fea maybe on side)
            self.ev_glog.record(self.main)

    def gather_log(self):
        # sync_log (the reference reads seven .item()s per step, SRRaGAN_model.py:171-186): round 5 — the host no longer
        # waits for the END of the step.  The seven scalars are gathered and copied to pinned memory on the side stream
        # right behind the D step's loss kernel (ev_log); the tail is enqueued first, THEN the host waits for
        # ev_log only (`read_log`): it returns ~1.3 ms of GPU work early and enqueues the next step under the rest of
        # this one (8.1 -> ~7 ms per step for a loop that logs every step).
        if self.ev_glog is None:
            return
        st, side = self.st, self.side
        with torch.cuda.stream(side):
            side.wait_event(self.ev_glog)
            if st._log_host is None:
                st._log_host = torch.empty(len(LOG_KEYS), dtype=torch.float32).pin_memory()
            self.log_keep = torch.stack([t.detach().reshape(()).float() for t in
                                         _log_values(self.l_g_pix, self.l_g_fea, self.l_g_gan, self.aux)])
            st._log_host.copy_(self.log_keep, non_blocking=True)
            self.ev_log = torch.cuda.Event()
            self.ev_log.record(side)

    def tail_on_main(self):
        st, side = self.st, self.side
        st._tail_on_main(self.main, side)
        if side is not None:
            st._ev_tail = torch.cuda.Event()
            st._ev_tail.record(side)
            st._defer_networks(st._ev_tail)

    def read_log(self):
        st = self.st
        if not self.sync_log:
            st.log = dict(zip(LOG_KEYS, _log_values(self.l_g_pix, self.l_g_fea, self.l_g_gan, self.aux)))
        elif self.ev_log is not None:
            self.ev_log.synchronize()                         # the losses, not the end of the step
            st.log = dict(zip(LOG_KEYS, st._log_host.tolist()))
            self.log_keep = None
            # the default call's contract: everything it enqueued is ordered on the CURRENT stream when it returns
            self.main.wait_event(st._ev_tail)
        else:                                                 # (no side stream: everything is on the current stream)
            st.log = {k: float(v) for k, v in
                      zip(LOG_KEYS, _log_values(self.l_g_pix, self.l_g_fea, self.l_g_gan, self.aux))}
        return st.log


class _SRGANPass(_GANPass):
    """`SRGANStep`'s own on a G-update iteration: `GANLoss` against constant labels, the THIRD netD call's update of
    the running statistics, a tail that is all on the main stream when it cannot be split, and the log left on the
    device for `SRGANStep.step`."""

    join_netd = True

    def g_gan_loss(self, out, grad_fake):
        st = self.st
        return LS.gan_raw(out[:self.n], True, st.gan_type, st.l_gan_w, grad_x=grad_fake,
                          grad_scale=self.S, scale_dev=self.sdev)[0]

    def d_gan_loss(self, out, gyt):
        # SRGAN_model.py:137-160: netD(real) and netD(fake.detach()) are groups 1 and 0 of the iteration's ONE pass;
        # the first is the second call (its values, its buffer update), the second a THIRD call on unchanged weights
        n, gyt = self.n, gyt.view(-1)
        return LS.gan_raw(out[n:], True, self.st.gan_type, 1.0, grad_x=gyt[n:], y=out[:n], y_is_real=False,
                          grad_y=gyt[:n], grad_scale=self.S, scale_dev=self.sdev)[1]

    def d_restat(self, PD):
        return CN.group0_restat(PD, self.n)           # call three: fake again

    def in_sequence(self):
        self.netd_forward()
        self.netf_fake()

    def tail_on_main(self):
        self.st._adam(True)
        self.st._ev_tail = None

    def read_log(self):
        """-> (the G terms this step has, `aux`), device scalars.  The default call: the tail ordered on the current
        stream first."""
        st = self.st
        if self.sync_log and st._ev_tail is not None:
            self.main.wait_event(st._ev_tail)
        g = (('l_g_pix', self.l_g_pix), ('l_g_gan', self.l_g_gan), ('l_g_fea', self.l_g_fea))
        return {k: v for k, v in g if v is not None}, self.aux


class ESRGANPlusStep(_StepBase):
    def __init__(self, netG, netD, netF, lr_G=1e-4, lr_D=1e-4, beta1_G=0.9, beta1_D=0.9,
                 pixel_weight=1e-2, feature_weight=1.0, gan_weight=5e-3, loss_scale=1.0, data_parallel=None,
                 pixel_criterion='l1', feature_criterion='l1'):
        _check_channels('ESRGANPlusStep', netG, netD, netF)
        super().__init__(netG, loss_scale, data_parallel)
        self.netD, self.netF = netD, netF
        # 'l1' / 'l2' (SRRaGAN_model.py:31-53): the raw and the autograd form of each criterion's one launch
        self._pix_raw, self._pix_loss = LS.criterion(pixel_criterion)
        self._fea_raw, self._fea_loss = LS.criterion(feature_criterion)
        self.l_pix_w, self.l_fea_w, self.l_gan_w = pixel_weight, feature_weight, gan_weight
        self.optimizer_G, self.exG = self._optimizer(netG, [p for p in netG.parameters() if p.requires_grad], lr_G, beta1_G)
        self.optimizer_D, self.exD = self._optimizer(netD, netD.parameters(), lr_D, beta1_D)
        # ESR_SHARED_D=0: the D step runs its own forward pair (round 3) instead of re-using the G step's pass
        self.shared_d = os.environ.get('ESR_SHARED_D', '1') != '0'
        # netF(fake): forward, feature loss and input-gradient pass on the SIDE stream, next to netD's forward and its
        # G-step pass on the main stream (both hang off fake_H only; their two contributions to dL/d fake_H meet in one add)
        self.netf_side = os.environ.get('ESR_TRAIN_NETF_SIDE', '1') == '1'
        self.d_when = self._knob('ESR_TRAIN_DSTEP', 'last', ('first', 'mid', 'last'))       # see _GANPass.place_d_step
        # The logging form (sync_log=True: the host reads the losses every step and the call returns with the D-side tail
        # ordered on the caller's stream) wants the D step EARLY and the follower pass of G's weight gradients BIG: the main
        # stream waits for the side stream's tail at the end of the call, so what the D step gains by running late under the
        # backward chain is lost again.  Round 6, same box, ms per logging-form step (tools/train_marks.py sync, two runs):
        # last / 80 workgroups 7.06 / 7.02; first / 96: 6.90 / 7.02; first / 112: 6.65 / 6.68; mid / 112: 6.66 / 6.63; first /
        # 128: 6.59 / 6.66; mid / 128: 6.60 / 6.58.  An explicit ESR_TRAIN_DSTEP / ESR_BWD_FOLLOW_WGS rules both forms.
        self.d_when_sync = self._knob('ESR_TRAIN_DSTEP_SYNC', os.environ.get('ESR_TRAIN_DSTEP', 'mid'), ('first', 'mid', 'last'))
        fw = os.environ.get('ESR_TRAIN_SYNC_FOLLOW_WGS', '' if os.environ.get('ESR_BWD_FOLLOW_WGS') else '128')
        self.follow_wgs_sync = int(fw) if fw else None
        # netD's forward in two stages: the `real` half on the side stream under the generator's forward (its input is
        # known when the step starts), the `fake` half alone behind the generator (A/B knob, round 5)
        self.d_split = os.environ.get('ESR_TRAIN_DSPLIT', '1') == '1'

    validate = _validate
    validate_hr = _validate_hr

    def _manual_ok(self):
        netG, netD, netF = self.netG, self.netD, self.netF
        return (self.manual and self.shared_d and getattr(netD, '_shared_ok', False) and netD.training
                and getattr(netG, 'flat_param_grads', False) and hasattr(netG, '_convs') and hasattr(netF, '_run_forward')
                and all(p.requires_grad for p in netG._convs()[1]) and all(p.requires_grad for p in netD.parameters()))

    def _step_manual(self, var_L, var_H, var_ref, z, sync_log):
        """optimize_parameters (SRRaGAN_model.py:113-168) as a hand-written forward / backward over the networks'
        launch lists — no autograd graph.  The same kernels in the same order as the autograd form of ``step`` (which
        stays for networks this path does not cover, and as the A/B reference: tests run both against the reference's
        golden steps); what disappears is the glue between them:
          * every loss kernel writes its gradient straight into the buffer the next backward list reads
            (losses.l1_raw / ragan_raw: the loss scale rides in the kernel);
          * dL/d fake_H = d l_pix + d l_fea + d l_gan is never summed by a launch: the pixel loss writes the buffer, the
            last layout ops of netF's and netD's input-gradient passes ADD into it (esr_layout.accumulate);
          * netD's parameter gradients stay in its plan's flat buffer (the parameters' .grad are persistent views of
            it: FusedAdam reads them in place); RRDBNet's leave the backward as one flat buffer which the parameters'
            `.grad` alias (`_deliver_flat_grads(adopt=True)`: no copy) and FusedAdam reads in place.
        The phases are `_ESRGANPass`'s methods; the order below is the order in which the HOST enqueues them."""
        p = _ESRGANPass(self, var_L, var_H, var_ref, z, sync_log)
        self._zero_stale_grads()
        p.mark('start')
        with torch.no_grad():
            p.generator_forward()
            p.under_generator_forward()
            p.pixel_loss()
            p.feature_and_gan_forward()
            p.fork_d_step()
            p.place_d_step('first')
            p.input_gradients()
            p.place_d_step('mid')
            p.generator_backward()
            p.place_d_step('last')
            p.release()
            p.gather_log()
            p.tail()
        return p.read_log()

    def _tail_on_main(self, main, side):
        """The step's tail ordered on the main stream, behind both backward passes: the two optimizer steps (each
        behind its gradient exchange), the loss scaler's update, and the next step's weight packs, now: the generator's
        forward copy on the main stream (the step starts with it anyway), everything that is only needed later — D's two
        packs, G's input-gradient operands — on the side stream (side=None: inline), next to it and to the start of the
        next generator forward."""
        inv = 1.0 / self.loss_scale          # the loss-scale division rides inside the Adam kernel
        self.exG.wait()
        self.optimizer_G.step(grad_scale=inv, scaler=self.scaler)
        self.exD.wait()
        self.optimizer_D.step(grad_scale=inv, scaler=self.scaler)
        if self.scaler:
            self.scaler.update()
        self.netG.prepack(fwd=True, dgrad=False)
        if side is not None:
            side.wait_stream(main)
            with torch.cuda.stream(side):
                self.netD.prepack()
                self.netG.prepack(fwd=False, dgrad=True)
        else:
            self.netD.prepack()
            self.netG.prepack(fwd=False, dgrad=True)

    def step(self, var_L, var_H, var_ref=None, z=None, sync_log=True):
        """One optimisation step (SRRaGAN_model.py:113-168).  sync_log=False: the pipelined form for training loops —
        the logged losses stay device tensors and the step's discriminator-side tail may still be in flight on the side
        stream when the call returns (the next step, ``finish()`` and a device synchronisation order it)."""
        netG, netD, netF = self.netG, self.netD, self.netF
        var_ref = var_H if var_ref is None else var_ref
        self._steps += 1
        E.require_cuda(var_L, 'ESRGANPlusStep.step: var_L')      # (the networks and the fused losses have no CPU path)
        if self._manual_ok():
            return self._step_manual(var_L, var_H, var_ref, z, sync_log)
        # batch means of the relativistic terms: over ALL ranks when data-parallel (losses._RaGANGlobalFn: the fused
        # kernel + two scalar all-reduces), else inside the one fused loss launch
        mean = self.data_parallel
        main = side = None
        # ---------------- G ----------------
        for p in netD.parameters():
            p.requires_grad = False
        self._zero_stale_grads()
        if self.overlap >= 1:
            # netF(var_H) does not depend on G: on the second stream, under the generator's forward
            main = torch.cuda.current_stream()
            side = self._side(var_L.device)
            side.wait_stream(main)
            with torch.cuda.stream(side), torch.no_grad():
                real_fea = netF(var_H)
            real_fea.record_stream(main)
        fake_H = self.fake_H = self._generator(var_L, z)
        l_g_pix = self._pix_loss(fake_H, var_H, self.l_pix_w)
        if side is not None:
            # join BEFORE netF runs on the main stream: the first netF call of a process packs its weights on the
            # side stream, and the side work finished under the generator's forward anyway
            main.wait_stream(side)
            fake_fea = netF(fake_H)
        else:
            fake_fea, real_fea = netF.forward_pair(fake_H, var_H)
        l_g_fea = self._fea_loss(fake_fea, real_fea, self.l_fea_w)
        # both operands in ONE pass (forward_pair: per-half BatchNorm statistics, the detached ``real`` half
        # costs no backward) — the reference's call order fake, real is the group order.  shared: the same pass
        # also keeps what the D step's pair needs (forward_shared), so that pair costs no second forward
        shared = None
        if self.shared_d and getattr(netD, '_shared_ok', False) and netD.training:
            pg, pr, shared = netD.forward_shared(fake_H, var_ref)
        else:
            pg, pr = netD.forward_pair(fake_H, var_ref)
        l_g_gan = LS.ragan_loss(pr, pg, False, True, self.l_gan_w, mean)[0]
        scale = self._scale(fake_H.device)
        aux = self._backward_autograd((l_g_pix, l_g_fea, l_g_gan), fake_H, var_ref, shared, scale, main, side)
        # (with overlap: the side stream's packs are joined at the next step's `main.wait_stream(side)` in front of
        # netF(fake_H): before any consumer)
        self._tail_on_main(main, side)
        logs = zip(LOG_KEYS, _log_values(l_g_pix, l_g_fea, l_g_gan, aux))
        if sync_log:      # the reference calls .item() on every loss each step (SRRaGAN_model.py:171-186)
            self.log = {k: float(v.detach()) for k, v in logs}
        else:
            self.log = {k: v.detach() for k, v in logs}
        return self.log

    def _backward_autograd(self, g_losses, fake_H, var_ref, shared, scale, main, side):
        """The G backward — d(scale * (pix + fea + gan)): one backward over the three terms, no sum / multiply launches —
        and the D step, each followed by the start of its gradient exchange; returns the D step's `aux`."""
        g_losses, scales = list(g_losses), [scale] * len(g_losses)
        if side is not None:
            # The D step does not depend on the G backward: it runs on a second stream UNDER it (both are chains of
            # small launches).  Same arithmetic, same order of BatchNorm running-statistics updates (its forward
            # still follows the G step's D pass); the autograd graphs are disjoint.  Data-parallel runs take the
            # same route: every rank issues its collectives in the same program order (D's loss sums, D's gradient
            # buckets on the side stream; G's in-backward buckets on the main stream), each stream-ordered after
            # the kernels that feed it.
            side.wait_stream(main)
            with torch.cuda.stream(side):
                aux = self._d_step_autograd(fake_H, var_ref, shared, scale)
                self.exD.start()
            torch.autograd.backward(g_losses, scales)
            self.exG.start()
            main.wait_stream(side)
        else:
            torch.autograd.backward(g_losses, scales)
            self.exG.start()                  # RCCL all-reduce of G grads overlaps the D pass below
            aux = self._d_step_autograd(fake_H, var_ref, shared, scale)
            self.exD.start()
        return aux

    def _d_step_autograd(self, fake_H, var_ref, shared, scale):
        # ---------------- D ---------------- (SRRaGAN_model.py:143-168; only needs fake_H's VALUES and D as it is)
        netD = self.netD
        for p in netD.parameters():
            p.requires_grad = True
        self.optimizer_D.zero_grad(set_to_none=True)
        if shared is not None:
            pred_d_real, pred_d_fake = shared.second_pass()
        else:
            with netD.weights_unchanged():        # no optimizer step since the G step's D pass
                pred_d_real, pred_d_fake = netD.forward_pair(var_ref, fake_H.detach())
        l_d_total, aux = LS.ragan_loss(pred_d_real, pred_d_fake, True, False, 1.0, self.data_parallel)
        torch.autograd.backward([l_d_total], [scale])
        return aux


class PSNRStep(_StepBase):
    """The PSNR-oriented pretraining step — ``SRModel.optimize_parameters`` (codes/models/SR_model.py:66-74) with the
    set-up of its constructor (SR_model.py:24-53; codes/options/train/train_sr.json): one pixel criterion ('l1' /
    'l2') on the generator's output, Adam(lr_G, weight_decay_G) over the parameters that train.  Stage one of the
    ESRGAN+ recipe: its result is the `pretrain_model_G` that ``ESRGANPlusStep`` fine-tunes.

    Production form (``netG.flat_param_grads``, every parameter trains): the generator's launch lists driven directly,
    the phases of bench.py's generator loop — training forward, ONE loss launch that also writes dL/d fake_H (times the
    loss scale) into a persistent buffer, backward, gradient exchange, fused Adam (which divides the scale out), loss
    scaler update, weight packs.  Beside the main stream: the backward's step-independent preliminaries
    (``functional.rrdbnet_train_prepare``) run on the side stream under the forward, and the input-gradient weight
    packs — which only the NEXT backward reads — follow the Adam update there.  Autograd form (ESR_TRAIN_MANUAL=0, a
    frozen parameter, a network without the flat gradient route): ``netG(var_L)``, the criterion's autograd face,
    ``torch.autograd.backward`` with the scale."""

    _nets = ('G',)
    follow_wgs_sync = None             # (the generator's backward as its plan sizes it)

    def __init__(self, netG, lr_G=2e-4, weight_decay_G=0, beta1_G=0.9, pixel_criterion='l1', pixel_weight=1.0,
                 loss_scale=1.0, data_parallel=None):
        super().__init__(netG, loss_scale, data_parallel)
        self._pix_raw, self._pix_loss = LS.criterion(pixel_criterion)
        self.l_pix_w = pixel_weight
        # "can optimize for a part of the model" (SR_model.py:40-44): a frozen parameter is left out
        self.optimizer_G, self.exG = self._optimizer(netG, [p for p in netG.parameters() if p.requires_grad], lr_G,
                                                     beta1_G, weight_decay_G if weight_decay_G else 0)
        self._gys = {}                     # dL/d fake_H, one buffer per (shape, device): mixed LR buckets alternate

    validate = _validate
    validate_hr = _validate_hr

    def _manual_ok(self):
        netG = self.netG
        return (self.manual and getattr(netG, 'flat_param_grads', False) and hasattr(netG, '_convs')
                and all(p.requires_grad for p in netG._convs()[1]))

    def _grad_buffer(self, fake):
        key = (tuple(fake.shape), fake.device)
        gy = self._gys.get(key)
        if gy is None:
            gy = self._gys[key] = torch.empty_like(fake)
        return gy

    def _step_manual(self, var_L, real_H, z, sync_log):
        p = _PSNRPass(self, var_L, real_H, z, sync_log)
        self._zero_stale_grads()
        with torch.no_grad():
            p.generator_forward()
            p.under_generator_forward()
            p.pixel_loss()
            p.generator_backward()
            p.tail()
        return p.read_log()

    def step(self, var_L, real_H, z=None, sync_log=True):
        """One optimisation step (SR_model.py:66-74).  sync_log=False: the pipelined form — ``l_pix`` stays a device
        tensor and the input-gradient weight packs may still be in flight on the side stream when the call returns
        (the next step, ``finish()``, the generator's public entry points and a device synchronisation order them)."""
        netG = self.netG
        self._steps += 1
        E.require_cuda(var_L, 'PSNRStep.step: var_L')         # (the generator and the fused losses have no CPU path)
        if self._manual_ok():
            return self._step_manual(var_L, real_H, z, sync_log)
        self._zero_stale_grads()
        fake_H = self.fake_H = self._generator(var_L, z)
        l_pix = self._pix_loss(fake_H, real_H, self.l_pix_w)
        torch.autograd.backward([l_pix], [self._scale(fake_H.device)])
        self.exG.start()
        self.exG.wait()
        self.optimizer_G.step(grad_scale=1.0 / self.loss_scale, scaler=self.scaler)
        if self.scaler:
            self.scaler.update()
        if hasattr(netG, 'prepack'):
            netG.prepack(fwd=True, dgrad=True)
        self.log = {'l_pix': float(l_pix.detach()) if sync_log else l_pix.detach()}
        return self.log


class SRGANStep(_StepBase):
    """The standard-GAN step — ``SRGANModel.optimize_parameters`` (codes/models/SRGAN_model.py:113-178) with the set-up
    of its constructor (SRGAN_model.py:29-98; codes/options/train/train_SRGAN.json): optional pixel and feature terms
    ('l1' / 'l2'; a weight <= 0 removes the term and its log key, and ``netF`` may then be None), ``GANLoss(gan_type)``
    ('vanilla' / 'lsgan') against constant labels, Adam for G and D with optional weight decay, and the update schedule
    of ``D_update_ratio`` / ``D_init_iters``: G moves when ``iteration % D_update_ratio == 0 and iteration >
    D_init_iters``, D every iteration.  ``iteration`` counts from 1 (the reference passes ``current_step``); left out, an
    internal counter supplies it, which ``state_dict()`` carries and ``checkpoint.resume_step`` restores.

    netD's BatchNorm buffers see the reference's calls in the reference's order: fake, real, fake on a G-update
    iteration (three momentum updates, ``num_batches_tracked`` + 3), real, fake otherwise.

    Hand-driven form (an ``RRDBNet`` generator with flat gradients, every parameter training — ``_manual_ok``): the
    networks' launch lists driven directly.  On a G-update iteration netD runs ONCE over [fake; real] (the dual plan of
    ``ESRGANPlusStep``): its second pass gives dL/d fake_H for G, its own pass D's parameter gradients, and the third
    call's buffer update is a replay on group 0 (``convnet.group0_restat``); the loss kernels write their gradients
    straight into the buffers the backward lists read.  Other iterations: the noise-on forward without saved
    activations and ``netD.forward_pair(var_ref, fake)``.  Autograd form (every other generator — ``SRResNet``, the
    generator of train_SRGAN.json —, a frozen parameter, ESR_TRAIN_MANUAL=0): the reference's three netD calls.

    Data-parallel: the losses are per-sample means, so per-rank losses and the averaged gradients reproduce the global
    batch's step; no scalar crosses the ranks.  The logged ``l_*`` / ``D_real`` / ``D_fake`` are this rank's means."""

    # The policy of the shared phases, fixed (no knobs).  The D step under the generator's backward on the side stream:
    # enqueued behind it by a loop that reads nothing (the host then feeds the main stream first), in front of it by
    # one that waits for the log; netF(fake) next to netD's forward; netD's `real` half under the generator's forward;
    # the generator's backward as its plan sizes it.
    d_when, d_when_sync = 'last', 'mid'
    netf_side = d_split = True
    follow_wgs_sync = None

    def __init__(self, netG, netD, netF=None, lr_G=1e-4, lr_D=1e-4, beta1_G=0.9, beta1_D=0.9,
                 weight_decay_G=0, weight_decay_D=0, pixel_weight=1e-2, feature_weight=1.0, gan_weight=5e-3,
                 pixel_criterion='l1', feature_criterion='l1', gan_type='vanilla',
                 D_update_ratio=1, D_init_iters=0, loss_scale=1.0, data_parallel=None):
        self.l_pix_w = pixel_weight if pixel_weight and pixel_weight > 0 else 0
        self.l_fea_w = feature_weight if feature_weight and feature_weight > 0 else 0
        self.l_gan_w = gan_weight
        self._pix_raw, self._pix_loss = LS.criterion(pixel_criterion) if self.l_pix_w else (None, None)
        self._fea_raw, self._fea_loss = LS.criterion(feature_criterion) if self.l_fea_w else (None, None)
        if self.l_fea_w and netF is None:
            raise ValueError('SRGANStep: feature_weight > 0 needs netF')
        self.netD, self.netF = netD, netF if self.l_fea_w else None
        _check_channels('SRGANStep', netG, netD, self.netF)
        self.gan_type = str(gan_type).lower()
        LS.gan_kind(self.gan_type)                # refuses 'wgan-gp' and unknown names
        self.D_update_ratio = int(D_update_ratio) if D_update_ratio else 1
        self.D_init_iters = int(D_init_iters) if D_init_iters else 0
        super().__init__(netG, loss_scale, data_parallel)
        self.optimizer_G, self.exG = self._optimizer(netG, [p for p in netG.parameters() if p.requires_grad], lr_G,
                                                     beta1_G, weight_decay_G if weight_decay_G else 0)
        self.optimizer_D, self.exD = self._optimizer(netD, netD.parameters(), lr_D, beta1_D,
                                                     weight_decay_D if weight_decay_D else 0)
        self.iteration = 0                 # iterations done (the next default `iteration` is this + 1)
        self._g_log = {}                   # the last G update's l_g_* (the reference's log_dict keeps them)

    validate = _validate
    validate_hr = _validate_hr

    @staticmethod
    def g_update_due(iteration, D_update_ratio=1, D_init_iters=0):
        """SRGAN_model.py:119: does the generator move at this iteration (counted from 1)?"""
        return iteration % D_update_ratio == 0 and iteration > D_init_iters

    def _manual_ok(self):
        netG, netD, netF = self.netG, self.netD, self.netF
        return (self.manual and getattr(netD, '_shared_ok', False) and netD.training
                and not getattr(netD, '_per_call_weights', False)
                and getattr(netG, 'flat_param_grads', False) and hasattr(netG, '_convs')
                and (netF is None or hasattr(netF, '_run_forward'))
                and all(p.requires_grad for p in netG._convs()[1]) and all(p.requires_grad for p in netD.parameters()))

    def state_dict(self):
        """The two optimizers' states (base_model.py:65-74) and the iteration counter, behind whatever is in flight."""
        return dict(super().state_dict(), iter=self.iteration)

    # ---- the two forms ----
    def _adam(self, update_g):
        """Both forms' tail: the optimizer steps behind their exchanges, the scaler's update, the weight packs."""
        inv = 1.0 / self.loss_scale
        if update_g:
            self.exG.wait()
            self.optimizer_G.step(grad_scale=inv, scaler=self.scaler)
        self.exD.wait()
        self.optimizer_D.step(grad_scale=inv, scaler=self.scaler)
        if self.scaler:
            self.scaler.update()
        if update_g and hasattr(self.netG, 'prepack'):
            self.netG.prepack(fwd=True, dgrad=True)
        if hasattr(self.netD, 'prepack'):
            self.netD.prepack()

    def _step_d_only(self, var_L, var_ref, z):
        """An iteration on which nothing of G moves, in both forms: the noise-on forward without saved activations; the
        D step as two calls in one pass, all on the caller's stream (the networks' entry points join what the last
        iteration left on the side stream)."""
        with torch.no_grad():
            fake = self.fake_H = self._generator(var_L, z)
        aux = self._d_step_autograd(var_ref, fake, self._scale(fake.device))
        self._adam(False)
        return {}, aux

    def _step_manual(self, var_L, var_H, var_ref, z, update_g, sync_log):
        """One iteration over the networks' launch lists; returns the device scalars (g_terms, aux).
        A G-update iteration runs `_SRGANPass`'s phases, in the order in which the HOST enqueues them: those of
        ``ESRGANPlusStep`` without the gathered log."""
        if not update_g:
            return self._step_d_only(var_L, var_ref, z)
        p = _SRGANPass(self, var_L, var_H, var_ref, z, sync_log)
        self._zero_stale_grads()
        with torch.no_grad():
            p.generator_forward()
            p.under_generator_forward()
            p.pixel_loss()
            p.feature_and_gan_forward()
            p.fork_d_step()
            p.place_d_step('first')
            p.input_gradients()
            p.place_d_step('mid')
            p.generator_backward()
            p.place_d_step('last')
            p.release()
            p.tail()
        return p.read_log()

    def _d_step_autograd(self, var_ref, fake, scale):
        """SRGAN_model.py:137-160 as the reference calls it: netD(real), netD(fake.detach()) — one pass, BatchNorm
        statistics per call —, ``l_d_real + l_d_fake`` as one loss launch, backward; returns `aux`."""
        netD = self.netD
        for p in netD.parameters():
            p.requires_grad = True
        self.optimizer_D.zero_grad(set_to_none=True)
        with torch.enable_grad():
            pred_d_real, pred_d_fake = netD.forward_pair(var_ref, fake.detach())
            l_d_total, aux = LS.gan_pair_loss(pred_d_real, True, pred_d_fake, False, self.gan_type, 1.0)
        torch.autograd.backward([l_d_total], [scale])
        self.exD.start()
        return aux

    def _step_autograd(self, var_L, var_H, var_ref, z, update_g, sync_log):
        netD, netF = self.netD, self.netF
        self._zero_stale_grads()
        if not update_g:
            return self._step_d_only(var_L, var_ref, z)
        g = {}
        for p in netD.parameters():                   # G's pass through netD: parameters frozen
            p.requires_grad = False
        fake_H = self.fake_H = self._generator(var_L, z)
        scale = self._scale(fake_H.device)
        if self.l_pix_w:
            g['l_g_pix'] = self._pix_loss(fake_H, var_H, self.l_pix_w)
        if self.l_fea_w:
            fake_fea, real_fea = netF.forward_pair(fake_H, var_H)
            g['l_g_fea'] = self._fea_loss(fake_fea, real_fea.detach(), self.l_fea_w)
        g['l_g_gan'] = LS.gan_loss(netD(fake_H), True, self.gan_type, self.l_gan_w)
        terms = list(g.values())
        torch.autograd.backward(terms, [scale] * len(terms))
        self.exG.start()
        with netD.weights_unchanged() if hasattr(netD, 'weights_unchanged') else contextlib.nullcontext():
            aux = self._d_step_autograd(var_ref, fake_H, scale)
        self._adam(True)
        return {k: v.detach() for k, v in g.items()}, aux

    def step(self, var_L, var_H, var_ref=None, z=None, sync_log=True, iteration=None):
        """One iteration (SRGAN_model.py:113-178).  sync_log=False: the pipelined form — the logged values stay device
        tensors and nothing waits for the host (the next step, ``finish()`` and a device synchronisation order what is
        in flight)."""
        E.require_cuda(var_L, 'SRGANStep.step: var_L')        # (the networks and the fused losses have no CPU path)
        var_ref = var_H if var_ref is None else var_ref
        it = self.iteration + 1 if iteration is None else int(iteration)
        self.iteration = it
        self._steps += 1
        update_g = self.g_update_due(it, self.D_update_ratio, self.D_init_iters)
        form = self._step_manual if self._manual_ok() else self._step_autograd
        g, aux = form(var_L, var_H, var_ref, z, update_g, sync_log)
        # the log: G's entries only change when G moves (log_dict keeps the last ones); aux = l_d_real, l_d_fake, D_real, D_fake
        vals = dict(g)
        vals.update(zip(('l_d_real', 'l_d_fake', 'D_real', 'D_fake'), aux.unbind(0)))
        if sync_log:
            keys = list(vals)
            host = torch.stack([vals[k].reshape(()).float() for k in keys]).tolist()       # one copy, one wait
            vals = dict(zip(keys, host))
        if update_g:
            self._g_log = {k: vals[k] for k in g}
        elif sync_log:
            self._g_log = {k: float(v) for k, v in self._g_log.items()}
        merged = dict(self._g_log)
        merged.update({k: vals[k] for k in ('l_d_real', 'l_d_fake', 'D_real', 'D_fake')})
        self.log = {k: merged[k] for k in LOG_KEYS if k in merged}
        return self.log
