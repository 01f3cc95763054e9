"""The ESRGAN+ train step's losses as single launches (csrc/loss_kernels.hip): ``nn.L1Loss`` / ``nn.MSELoss`` (cri_pix /
cri_fea 'l1' / 'l2', SRRaGAN_model.py:31-53,124-131; SR_model.py:28-34) and the relativistic-average GAN term built from ``GANLoss('vanilla')``
(codes/models/modules/loss.py:6-38; SRRaGAN_model.py:133-137, 150-156), and ``GANLoss`` itself ('vanilla' / 'lsgan'
against a constant label: SRGAN_model.py:129-146).  Each forward launch also produces the
gradient w.r.t. its differentiable operands; backward is one multiply by the upstream scalar.

Same numbers as the torch formulas (tests/test_gpu_losses.py).  No fallback: operands the kernels do not cover (CPU
tensors, non-fp32, shape mismatch, a target that needs a gradient) raise ``HipExtensionError``; non-contiguous or
16-byte-misaligned views are handled (a contiguous copy / the kernel's scalar path).  Data-parallel runs keep the
relativistic means GLOBAL: the same kernel in three modes with two scalar all-reduces in between
(``ragan_loss(..., global_mean=True)``).
"""
import ctypes as C

import torch

from . import _lib as L
from . import engine as E
from . import dp as DP

_scratch = {}


def _dev_scratch(dev):
    t = _scratch.get(dev)
    if t is None:
        t = _scratch[dev] = torch.zeros(2, dtype=torch.float64, device=dev)
    return t


def _require(ok, what):
    if not ok:
        raise L.HipExtensionError('esrganplus_amd.losses: ' + what + ' (the fused loss kernels take fp32 tensors on '
                                  'the MI355X; there is no torch fallback)')


def _check_operands(name, *ts):
    for t in ts:
        _require(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32,
                 '%s: operand is %s / %s' % (name, getattr(t, 'device', type(t)), getattr(t, 'dtype', '')))


class _PixelFn(torch.autograd.Function):
    """The autograd face of one pixel-loss entry (`entry`: 'esr_l1_loss_forward' / 'esr_l2_loss_forward')."""

    @staticmethod
    def forward(ctx, a, b, weight, entry):
        a_, b_ = a.detach().contiguous(), b.detach().contiguous()
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        grad = torch.empty_like(a_) if ctx.needs_input_grad[0] else None
        p = L.esr_l1_loss()
        p.a, p.b, p.loss, p.n, p.weight = a_.data_ptr(), b_.data_ptr(), loss.data_ptr(), a_.numel(), weight
        p.grad_a = grad.data_ptr() if grad is not None else None
        p.scratch = _dev_scratch(a.device).data_ptr()
        L.check(getattr(L.lib(), entry)(C.byref(p), C.c_void_p(E.current_stream())), entry)
        ctx.grad = grad
        return loss

    @staticmethod
    def backward(ctx, g):
        return (ctx.grad * g if ctx.grad is not None else None), None, None, None


def _as_f32(t):
    # fp16 / bf16 operands (an autocast caller): upcast — autograd carries the gradient back through the cast
    return t.float() if torch.is_tensor(t) and t.is_cuda and t.dtype in (torch.float16, torch.bfloat16) else t


def _scale_args(p, grad_scale, scale_dev):
    p.grad_scale = float(grad_scale)
    if scale_dev is not None:
        p.grad_scale_dev = scale_dev.data_ptr()


def _pixel_raw(name, entry, a, b, weight, grad_out, grad_scale, scale_dev):
    a_, b_ = a.detach().contiguous(), b.detach().contiguous()
    _check_operands(name, a_, b_)
    _require(a_.shape == b_.shape, '%s: shapes %s vs %s' % (name, tuple(a_.shape), tuple(b_.shape)))
    loss = torch.empty((), dtype=torch.float32, device=a_.device)
    p = L.esr_l1_loss()
    p.a, p.b, p.loss, p.n, p.weight = a_.data_ptr(), b_.data_ptr(), loss.data_ptr(), a_.numel(), float(weight)
    if grad_out is not None:
        _require(grad_out.is_contiguous() and grad_out.dtype == torch.float32 and grad_out.numel() == a_.numel(), name + ': grad_out')
        p.grad_a = grad_out.data_ptr()
    p.scratch = _dev_scratch(a_.device).data_ptr()
    _scale_args(p, grad_scale, scale_dev)
    L.check(getattr(L.lib(), entry)(C.byref(p), C.c_void_p(E.current_stream())), entry)
    return loss


def l1_raw(a, b, weight, grad_out=None, grad_scale=1.0, scale_dev=None):
    """One launch, no autograd: ``(weight * mean|a - b|, grad)`` with ``grad = grad_scale [* scale_dev[0]] * weight *
    sign(a - b) / n`` written into ``grad_out`` (a contiguous fp32 tensor of a's size — e.g. the buffer a backward launch
    list reads its upstream gradient from) or not formed at all (``grad_out=None``).  The hand-written train step
    (train.ESRGANPlusStep) calls the losses this way; ``l1_loss`` is the autograd face of the same kernel."""
    return _pixel_raw('l1_raw', 'esr_l1_loss_forward', a, b, weight, grad_out, grad_scale, scale_dev)


def l2_raw(a, b, weight, grad_out=None, grad_scale=1.0, scale_dev=None):
    """``l1_raw`` for ``nn.MSELoss``: ``weight * mean (a - b)^2`` with ``grad = grad_scale [* scale_dev[0]] * weight *
    2 (a - b) / n`` into ``grad_out`` (None: not formed).  One launch, the device scratch of ``l1_raw``."""
    return _pixel_raw('l2_raw', 'esr_l2_loss_forward', a, b, weight, grad_out, grad_scale, scale_dev)


def ragan_raw(x, y, x_is_real, y_is_real, weight, grad_x=None, grad_y=None, grad_scale=1.0, scale_dev=None,
              global_mean=False):
    """The relativistic-average GAN term without autograd: ``(loss, aux)`` as ``ragan_loss``; the gradients w.r.t. the
    logits, times ``grad_scale [* scale_dev[0]]``, are written into ``grad_x`` / ``grad_y`` (contiguous fp32, n floats;
    None: not formed).  ``global_mean``: the batch means run over all ranks (two scalar all-reduces between the launches,
    as ``_RaGANGlobalFn``)."""
    import torch.distributed as dist
    x_, y_ = x.detach().contiguous().view(-1), y.detach().contiguous().view(-1)
    _check_operands('ragan_raw', x_, y_)
    _require(x_.numel() == y_.numel(), 'ragan_raw: %d vs %d logits' % (x_.numel(), y_.numel()))
    dev = x_.device
    st = C.c_void_p(E.current_stream())
    loss = torch.empty((), dtype=torch.float32, device=dev)
    out = torch.empty(4, dtype=torch.float32, device=dev)        # mean(x), mean(y), BCE_x, BCE_y
    p = L.esr_ragan_loss()
    p.x, p.y, p.n = x_.data_ptr(), y_.data_ptr(), x_.numel()
    p.tx, p.ty, p.weight = (1.0 if x_is_real else 0.0), (1.0 if y_is_real else 0.0), float(weight)
    p.loss, p.mean_x, p.mean_y = loss.data_ptr(), out.data_ptr(), out.data_ptr() + 4
    p.bce_x, p.bce_y = out.data_ptr() + 8, out.data_ptr() + 12
    _scale_args(p, grad_scale, scale_dev)
    gx = grad_x.data_ptr() if grad_x is not None else None
    gy = grad_y.data_ptr() if grad_y is not None else None
    if not (global_mean and DP.active()):
        p.grad_x, p.grad_y = gx, gy
        L.check(L.lib().esr_ragan_loss_forward(C.byref(p), st), 'esr_ragan_loss_forward')
        return loss, out
    ext = torch.zeros(5, dtype=torch.float32, device=dev)       # sum x, sum y, n | D1, D2 (all ranks)
    ext[2] = float(x_.numel())
    p.mode, p.sums = 1, ext.data_ptr()
    L.check(L.lib().esr_ragan_loss_forward(C.byref(p), st), 'esr_ragan_loss_forward')
    dist.all_reduce(ext[0:3])
    dsum = torch.zeros(2, dtype=torch.float32, device=dev)
    p.mode, p.sums, p.ext = 2, dsum.data_ptr(), ext.data_ptr()
    L.check(L.lib().esr_ragan_loss_forward(C.byref(p), st), 'esr_ragan_loss_forward')
    if gx is not None or gy is not None:
        dist.all_reduce(dsum)
        ext[3:5] = dsum
        p.mode, p.grad_x, p.grad_y = 3, gx, gy
        L.check(L.lib().esr_ragan_loss_forward(C.byref(p), st), 'esr_ragan_loss_forward')
    return loss, out


def _pixel_loss(name, entry, a, b, weight):
    a, b = _as_f32(a), _as_f32(b)
    _check_operands(name, a, b)
    _require(a.shape == b.shape, '%s: shapes %s vs %s' % (name, tuple(a.shape), tuple(b.shape)))
    _require(not b.requires_grad, name + ': the target must not require a gradient')
    return _PixelFn.apply(a, b, float(weight), entry)


def l1_loss(a, b, weight=1.0):
    """``weight * F.l1_loss(a, b)``; the gradient flows to ``a`` only (``b`` is the target: var_H / real_fea — a target
    that requires a gradient is refused, not silently detached).  fp16 / bf16 operands are upcast."""
    return _pixel_loss('l1_loss', 'esr_l1_loss_forward', a, b, weight)


def l2_loss(a, b, weight=1.0):
    """``weight * F.mse_loss(a, b)``, otherwise as ``l1_loss`` (gradient to ``a`` only, fp16 / bf16 upcast)."""
    return _pixel_loss('l2_loss', 'esr_l2_loss_forward', a, b, weight)


# the reference's criterion names (SR_model.py:28-34, SRRaGAN_model.py:31-53) -> (raw form, autograd form)
CRITERIA = {'l1': (l1_raw, l1_loss), 'l2': (l2_raw, l2_loss)}


def criterion(loss_type):
    """(raw, autograd) forms of the reference's ``pixel_criterion`` / ``feature_criterion`` names."""
    try:
        return CRITERIA[loss_type]
    except (KeyError, TypeError):
        raise NotImplementedError('Loss type [{:s}] is not recognized.'.format(str(loss_type))) from None


class _RaGANFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, tx, ty, weight):
        x_, y_ = x.detach().contiguous().view(-1), y.detach().contiguous().view(-1)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        out = torch.empty(4, dtype=torch.float32, device=x.device)        # mean(x), mean(y), BCE_x, BCE_y
        gx = torch.empty_like(x_) if ctx.needs_input_grad[0] else None
        gy = torch.empty_like(y_) if ctx.needs_input_grad[1] else None
        p = L.esr_ragan_loss()
        p.x, p.y, p.n = x_.data_ptr(), y_.data_ptr(), x_.numel()
        p.grad_x = gx.data_ptr() if gx is not None else None
        p.grad_y = gy.data_ptr() if gy is not None else None
        p.loss, p.mean_x, p.mean_y = loss.data_ptr(), out.data_ptr(), out.data_ptr() + 4
        p.bce_x, p.bce_y = out.data_ptr() + 8, out.data_ptr() + 12
        p.tx, p.ty, p.weight = tx, ty, weight
        L.check(L.lib().esr_ragan_loss_forward(C.byref(p), C.c_void_p(E.current_stream())), 'esr_ragan_loss_forward')
        ctx.g = (gx, gy, x.shape, y.shape)
        ctx.mark_non_differentiable(out)
        return loss, out

    @staticmethod
    def backward(ctx, g, _unused):
        gx, gy, sx, sy = ctx.g
        return ((gx * g).view(sx) if gx is not None else None, (gy * g).view(sy) if gy is not None else None,
                None, None, None)


class _RaGANGlobalFn(torch.autograd.Function):
    """The same loss with the batch means taken over ALL ranks (SRRaGAN_model.py:136-137,151-152: under the
    reference's DataParallel the loss is formed on the gathered outputs).  Three launches of the one
    kernel; between them the rank-local scalar sums are all-reduced: [sum x, sum y, n] before the loss,
    [sum (sigmoid(z1) - tx), sum (sigmoid(z2) - ty)] before the gradients (every rank's loss sees the means, and the
    parameter gradients are averaged over ranks afterwards — GradExchange — which together reproduce the gradient of
    the single global-batch loss)."""

    @staticmethod
    def forward(ctx, x, y, tx, ty, weight):
        import torch.distributed as dist
        x_, y_ = x.detach().contiguous().view(-1), y.detach().contiguous().view(-1)
        dev = x.device
        st = C.c_void_p(E.current_stream())
        ext = torch.zeros(5, dtype=torch.float32, device=dev)       # sum x, sum y, n | D1, D2 (all ranks)
        ext[2] = float(x_.numel())
        p = L.esr_ragan_loss()
        p.x, p.y, p.n = x_.data_ptr(), y_.data_ptr(), x_.numel()
        p.tx, p.ty, p.weight = tx, ty, weight
        p.mode, p.sums = 1, ext.data_ptr()
        L.check(L.lib().esr_ragan_loss_forward(C.byref(p), st), 'esr_ragan_loss_forward')
        if DP.active():
            dist.all_reduce(ext[0:3])
        loss = torch.empty((), dtype=torch.float32, device=dev)
        out = torch.empty(4, dtype=torch.float32, device=dev)
        dsum = torch.zeros(2, dtype=torch.float32, device=dev)
        p.mode, p.sums, p.ext = 2, dsum.data_ptr(), ext.data_ptr()
        p.loss, p.mean_x, p.mean_y = loss.data_ptr(), out.data_ptr(), out.data_ptr() + 4
        p.bce_x, p.bce_y = out.data_ptr() + 8, out.data_ptr() + 12
        L.check(L.lib().esr_ragan_loss_forward(C.byref(p), st), 'esr_ragan_loss_forward')
        ctx.need = (ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        ctx.keep = (x_, y_, ext, dsum, tx, ty, weight, x.shape, y.shape)
        ctx.mark_non_differentiable(out)
        return loss, out

    @staticmethod
    def backward(ctx, g, _unused):
        import torch.distributed as dist
        x_, y_, ext, dsum, tx, ty, weight, sx, sy = ctx.keep
        if DP.active():
            dist.all_reduce(dsum)
        ext[3:5] = dsum
        gx = torch.empty_like(x_) if ctx.need[0] else None
        gy = torch.empty_like(y_) if ctx.need[1] else None
        p = L.esr_ragan_loss()
        p.x, p.y, p.n = x_.data_ptr(), y_.data_ptr(), x_.numel()
        p.tx, p.ty, p.weight = tx, ty, weight
        p.mode, p.ext = 3, ext.data_ptr()
        p.grad_x = gx.data_ptr() if gx is not None else None
        p.grad_y = gy.data_ptr() if gy is not None else None
        L.check(L.lib().esr_ragan_loss_forward(C.byref(p), C.c_void_p(E.current_stream())), 'esr_ragan_loss_forward')
        return ((gx * g).view(sx) if gx is not None else None, (gy * g).view(sy) if gy is not None else None,
                None, None, None)


def ragan_loss(x, y, x_is_real, y_is_real, weight=1.0, global_mean=False):
    """``weight * (BCE(x - mean(y), x_is_real) + BCE(y - mean(x), y_is_real)) / 2`` and the two means
    (returned as ``(loss, aux)`` with ``aux = [mean_x, mean_y, BCE_x, BCE_y]``, detached).  ``global_mean``: the means
    run over the batch of ALL ranks (data-parallel training; == the local batch on one rank)."""
    x, y = _as_f32(x), _as_f32(y)
    _check_operands('ragan_loss', x, y)
    _require(x.numel() == y.numel(), 'ragan_loss: %d vs %d logits' % (x.numel(), y.numel()))
    fn = _RaGANGlobalFn if global_mean else _RaGANFn
    return fn.apply(x, y, 1.0 if x_is_real else 0.0, 1.0 if y_is_real else 0.0, float(weight))


# ---- GANLoss (codes/models/modules/loss.py:6-38): the standard-GAN criterion of SRGAN_model.py --------------------
GAN_KINDS = {'vanilla': 0, 'lsgan': 1}


def gan_kind(gan_type):
    """The kernel's `kind` of the reference's ``gan_type`` (lowered as GANLoss.__init__ lowers it)."""
    name = str(gan_type).lower()
    if name in GAN_KINDS:
        return GAN_KINDS[name]
    if name == 'wgan-gp':
        raise NotImplementedError('GAN type [wgan-gp] is not supported: its gradient penalty needs a double backward '
                                  'through the discriminator, which the planned networks do not have')
    raise NotImplementedError('GAN type [{:s}] is not found'.format(name))


def _gan_launch(x_, y_, tx, ty, kind, weight, gx, gy, grad_scale, scale_dev):
    dev = x_.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    aux = torch.empty(4, dtype=torch.float32, device=dev)         # term_x, term_y, mean_x, mean_y
    p = L.esr_gan_loss()
    p.x, p.n_x, p.tx = x_.data_ptr(), x_.numel(), float(tx)
    if y_ is not None:
        p.y, p.n_y, p.ty = y_.data_ptr(), y_.numel(), float(ty)
    p.kind, p.weight, p.loss = kind, float(weight), loss.data_ptr()
    p.term_x, p.term_y, p.mean_x, p.mean_y = (aux.data_ptr() + 4 * i for i in range(4))
    p.grad_x = gx.data_ptr() if gx is not None else None
    p.grad_y = gy.data_ptr() if gy is not None else None
    _scale_args(p, grad_scale, scale_dev)
    L.check(L.lib().esr_gan_loss_forward(C.byref(p), C.c_void_p(E.current_stream())), 'esr_gan_loss_forward')
    return loss, aux


def gan_raw(x, x_is_real, gan_type, weight, grad_x=None, y=None, y_is_real=None, grad_y=None, grad_scale=1.0,
            scale_dev=None, real_label_val=1.0, fake_label_val=0.0):
    """``GANLoss(gan_type, real_label_val, fake_label_val)`` without autograd, one launch: ``(loss, aux)`` with
    ``loss = weight * (l(x, x_is_real) [+ l(y, y_is_real)])`` and ``aux = [term_x, term_y, mean_x, mean_y]`` (the
    unweighted terms and the logits' means; zeros for an absent ``y``).  The gradients w.r.t. the logits, times ``weight
    * grad_scale [* scale_dev[0]]``, are written into ``grad_x`` / ``grad_y`` (contiguous fp32 of the operand's size;
    None: not formed).  The two operands may differ in size."""
    kind = gan_kind(gan_type)
    x_ = x.detach().contiguous().view(-1)
    y_ = y.detach().contiguous().view(-1) if y is not None else None
    _check_operands('gan_raw', *((x_,) if y_ is None else (x_, y_)))
    _require(x_.numel() >= 1 and (y_ is None or y_.numel() >= 1), 'gan_raw: an operand without elements')
    _require(y_ is None or y_is_real is not None, 'gan_raw: y without y_is_real')
    for name, g, t in (('grad_x', grad_x, x_), ('grad_y', grad_y, y_)):
        if g is not None:
            _require(t is not None and g.is_cuda and g.is_contiguous() and g.dtype == torch.float32
                     and g.numel() == t.numel(), 'gan_raw: ' + name)
    label = lambda real: real_label_val if real else fake_label_val
    return _gan_launch(x_, y_, label(x_is_real), label(y_is_real) if y_ is not None else 0.0, kind, weight,
                       grad_x, grad_y if y_ is not None else None, grad_scale, scale_dev)


class _GANFn(torch.autograd.Function):
    """The autograd face of esr_gan_loss_forward: y may be None (one operand)."""

    @staticmethod
    def forward(ctx, x, y, tx, ty, kind, weight):
        x_ = x.detach().contiguous().view(-1)
        y_ = y.detach().contiguous().view(-1) if y is not None else None
        gx = torch.empty_like(x_) if ctx.needs_input_grad[0] else None
        gy = torch.empty_like(y_) if y_ is not None and ctx.needs_input_grad[1] else None
        loss, aux = _gan_launch(x_, y_, tx, ty, kind, weight, gx, gy, 1.0, None)
        ctx.g = (gx, gy, x.shape, y.shape if y is not None else None)
        ctx.mark_non_differentiable(aux)
        return loss, aux

    @staticmethod
    def backward(ctx, g, _unused):
        gx, gy, sx, sy = ctx.g
        return ((gx * g).view(sx) if gx is not None else None, (gy * g).view(sy) if gy is not None else None,
                None, None, None, None)


def gan_pair_loss(x, x_is_real, y, y_is_real, gan_type='vanilla', weight=1.0, real_label_val=1.0, fake_label_val=0.0):
    """``weight * (GANLoss(x, x_is_real) + GANLoss(y, y_is_real))`` as ONE launch with autograd — the D step's
    ``l_d_real + l_d_fake`` (SRGAN_model.py:140-146).  Returns ``(loss, aux)``, aux as ``gan_raw``, detached."""
    kind = gan_kind(gan_type)
    x, y = _as_f32(x), _as_f32(y)
    _check_operands('gan_pair_loss', x, y)
    _require(x.numel() >= 1 and y.numel() >= 1, 'gan_pair_loss: an operand without elements')
    label = lambda real: float(real_label_val if real else fake_label_val)
    return _GANFn.apply(x, y, label(x_is_real), label(y_is_real), kind, float(weight))


def gan_loss(x, target_is_real, gan_type='vanilla', weight=1.0, real_label_val=1.0, fake_label_val=0.0):
    """``weight * GANLoss(gan_type, real_label_val, fake_label_val)(x, target_is_real)``: one launch that also forms the
    gradient; backward is one multiply.  fp16 / bf16 logits are upcast."""
    kind = gan_kind(gan_type)
    x = _as_f32(x)
    _check_operands('gan_loss', x)
    _require(x.numel() >= 1, 'gan_loss: an operand without elements')
    t = float(real_label_val if target_is_real else fake_label_val)
    return _GANFn.apply(x, None, t, 0.0, kind, float(weight))[0]


class GANLoss(torch.nn.Module):
    """The reference's ``GANLoss`` (loss.py:6-38) over the fused kernel: same constructor, same ``forward(input,
    target_is_real)`` — a loop written against the reference keeps its ``self.cri_gan`` line."""

    def __init__(self, gan_type, real_label_val=1.0, fake_label_val=0.0):
        super().__init__()
        self.gan_type = str(gan_type).lower()
        gan_kind(self.gan_type)
        self.real_label_val, self.fake_label_val = real_label_val, fake_label_val

    def forward(self, input, target_is_real):
        return gan_loss(input, target_is_real, self.gan_type, 1.0, self.real_label_val, self.fake_label_val)
