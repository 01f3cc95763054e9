"""Kernel-side copies of the conv weights: the MFMA-fragment-ordered packs of the forward (WeightPack) and
input-gradient (DgradPack) operands, and the fused per-block weight streams that the dense-block chain kernels read,
gathered out of a pack's arena.  The fp32 OIHW nn.Parameters stay the master copy."""
import collections
import itertools

import torch

from . import _lib as L


def _dt(dtype):
    if dtype in ('fp16', torch.float16, L.ESR_F16):
        return L.ESR_F16, torch.float16, 16
    if dtype in ('fp32', torch.float32, L.ESR_F32):
        return L.ESR_F32, torch.float32, 8
    raise ValueError('dtype must be fp16 or fp32, got %r' % (dtype,))


def require_cuda(t, what):
    if not t.is_cuda:
        raise L.HipExtensionError(
            'esrganplus_amd: %s is on %s — the HIP path needs a CUDA/HIP tensor on an MI355X; '
            'there is no CPU fallback (use oracle/ for CPU reference results).' % (what, t.device))


class ConvW:
    """Packed weights of one conv (a slice of a pack's arena)."""
    __slots__ = ('key', 'cout', 'cin', 'ks', 'w_ptr', 'bias_ptr', 'has_bias', 'subpix')

    def __init__(self, key, cout, cin, ks, w_ptr, has_bias=False, subpix=False):
        self.key, self.cout, self.cin, self.ks, self.w_ptr = key, cout, cin, ks, w_ptr
        self.bias_ptr, self.has_bias, self.subpix = None, has_bias, subpix


class _Pack:
    """What WeightPack and DgradPack share: the arena, and ``ensure()``'s change detection — storages first (a sampled
    fingerprint, now and then every pointer; a change rebuilds the pack op list), then ``_version`` signatures (a
    change runs it).  A subclass sets ``self._watch`` (the flat list of tensors it packs from) and defines
    ``_packs()`` (its esr_pack list) and, if something runs besides the pack launch, ``_after_pack()``."""

    FULL_CHECK_EVERY = 64     # calls between full pointer comparisons (an unsampled parameter re-pointed by hand:
    #                            `p.data = t`, per-layer re-init, load_state_dict(assign=True))

    def __init__(self, dtype, device, specs, watch, folds=()):
        # specs: (key, cout, cin, ks, packed bytes) of every entry, in arena order
        # folds: (key, weight, bias or None) of nearest-x3 up-convs: the pack holds their folded form (esr_fold3: fp32
        # [9 cout, cin, 3, 3] + [9 cout]) as a derived tensor, refreshed by the launch list of every re-pack in front of
        # the pack launch, and packs it as entry key + '#fold'
        self.folded = {}
        for key, w, b in folds:
            self.folded[key] = (w, b, torch.zeros((9 * w.shape[0],) + tuple(w.shape[1:]), dtype=torch.float32, device=device),
                                torch.zeros(9 * w.shape[0], dtype=torch.float32, device=device) if b is not None else None)
        self.esr_dtype, self.tdtype, self.cpg = _dt(dtype)
        self.device = device
        self.arena = torch.zeros(sum(s[4] for s in specs), dtype=torch.uint8, device=device)
        offs = itertools.accumulate([0] + [s[4] for s in specs])
        self.entries = {s[0]: ConvW(*s[:4], self.arena.data_ptr() + off) for s, off in zip(specs, offs)}
        self._watch = watch
        # a few sampled storages + the count: parameters move together (.to / .cuda / DataParallel replicas); the full
        # per-tensor tuple (2 x ~390 data_ptr calls for the generator) costs ~0.2 ms of host time per training step
        n = len(watch)
        self._sampled = [watch[i] for i in sorted({0, n // 2, n - 1}) if 0 <= i < n]
        self._calls = 0
        self._fp = self._ptrs = self._sig = self.ops = None
        self.generation = 0      # bumped when any pointer handed out may have changed (plan caches key on it)
        self.pack_count = 0      # bumped every time the arena is re-packed (the weight streams re-gather)

    def _pack_op(self, w, dst, ks, **fields):
        pk = L.esr_pack()
        pk.src, pk.dst = w.data_ptr(), dst
        pk.cout, pk.cin, pk.ks = w.shape[0], w.shape[1], ks
        pk.dtype = self.esr_dtype
        for name, v in fields.items():
            setattr(pk, name, v)
        return pk

    def _after_pack(self):
        pass

    def ensure(self, stream, force=False, record_sig=False, full=False):
        """Re-pack when a watched tensor's storage or version changed, or unconditionally when ``force``.
        full=True (the module saw load_state_dict / _apply / replicate): compare EVERY storage, not the sampled
        fingerprint; the same happens on every FULL_CHECK_EVERY-th call.
        record_sig: a forced pack whose result a later non-forced call may rely on (_PlannedModule.prepack)."""
        fp = (len(self._watch),) + tuple(t.data_ptr() for t in self._sampled)
        self._calls += 1
        if full or self._calls % self.FULL_CHECK_EVERY == 0 or fp != self._fp:
            ptrs = tuple(t.data_ptr() for t in self._watch)
            if ptrs != self._ptrs:
                bp, self._pack_keep = L.batch_pack_op(self._packs(), self.device)
                self.ops = L.OpList()                      # ONE launch re-packs every conv of the network
                for w, b, wf, bf in self.folded.values():
                    f = L.esr_fold3()
                    f.mode, f.cout, f.cin = L.FOLD3_FOLD, w.shape[0], w.shape[1]
                    f.w, f.bias, f.wf, f.bf = w.data_ptr(), b.data_ptr() if b is not None else None, wf.data_ptr(), \
                        bf.data_ptr() if bf is not None else None
                    self.ops.add(L.OP_FOLD3, 'fold3', f)
                self.ops.add(L.OP_PACK_BATCH, 'pack_batch', bp)
                self.generation += 1
                self._ptrs = ptrs
                self._sig = None
            self._fp = fp
        # training passes re-pack unconditionally (FusedAdam updates through raw pointers: no version bump to see)
        sig = None if (force and not record_sig) else tuple(t._version for t in self._watch)
        if force or sig != self._sig:
            self.ops.run(stream)
            self._after_pack()
            self._sig = sig
            self.pack_count += 1


class WeightPack(_Pack):
    """Forward operands of a module's convs; biases are read from the parameters themselves, except those of convs with
    cout % 32 != 0, which are copied into a padded arena behind every re-pack."""

    def __init__(self, convs, dtype, device, subpix=(), folds=()):
        # convs: list of (key, weight_param, bias_param_or_None); subpix: keys of up-convs (nearest x2 + 3x3,
        # block.py:315-322) packed in the 4-phase 2x2 form (esr_pack.ups_fwd, run with esr_conv.upsample = 3)
        # folds: keys of nearest-x3 up-convs, also packed in their folded form as key + '#fold' (_Pack.__init__)
        dt_e = _dt(dtype)[0]
        folds = [c for c in convs if c[0] in frozenset(folds)]
        self.subpix, self.convs = frozenset(subpix), convs
        specs = []
        for key, w, b in convs:
            cout, cin, ks, _ = w.shape
            if key in self.subpix:      # 4 phases x cout blocks, 2x2 taps
                nbytes = L.packed_weight_bytes(4 * 32 * ((cout + 31) // 32), cin, 2, dt_e)
            else:
                nbytes = L.packed_weight_bytes(cout, cin, ks, dt_e)
            specs.append((key, cout, cin, ks, nbytes))
        specs += [(key + '#fold', 9 * w.shape[0], w.shape[1], 3, L.packed_weight_bytes(9 * w.shape[0], w.shape[1], 3, dt_e))
                  for key, w, b in folds]
        super().__init__(dtype, device, specs, [p for _, w, b in convs for p in (w, b) if p is not None], folds)
        nb_pad = sum(((w.shape[0] + 31) // 32) * 32 for _, w, b in convs if b is not None and w.shape[0] % 32)
        self.bias_arena = torch.zeros(max(nb_pad, 1), dtype=torch.float32, device=device)
        self._bias_copies = []
        bo = 0
        for key, w, b in convs:
            e = self.entries[key]
            e.has_bias, e.subpix = b is not None, key in self.subpix
            if b is not None and e.cout % 32:      # (cout % 32 == 0: _packs points bias_ptr at the parameter itself)
                e.bias_ptr = self.bias_arena.data_ptr() + 4 * bo
                self._bias_copies.append((b, self.bias_arena[bo:bo + e.cout]))
                bo += ((e.cout + 31) // 32) * 32

    def _packs(self):
        packs = []
        for key, w, b in self.convs:
            for p in (w, b):
                if p is not None:
                    require_cuda(p, 'parameter ' + key)
                    if p.dtype != torch.float32 or not p.is_contiguous():
                        raise L.HipExtensionError('parameter %s must be contiguous fp32 (master weights)' % key)
            e = self.entries[key]
            packs.append(self._pack_op(w, e.w_ptr, e.ks, ups_fwd=1 if e.subpix else 0))
            if b is not None and e.cout % 32 == 0:
                e.bias_ptr = b.data_ptr()
        for key, (w, b, wf, bf) in self.folded.items():
            e = self.entries[key + '#fold']
            packs.append(self._pack_op(wf, e.w_ptr, 3))
            e.has_bias, e.bias_ptr = bf is not None, bf.data_ptr() if bf is not None else None
        return packs

    def _after_pack(self):
        with torch.no_grad():
            for src, dst in self._bias_copies:
                dst.copy_(src)


class DgradPack(_Pack):
    """Packed operands of the input-gradient convolutions: Cin<->Cout transposed, taps rotated 180
    degrees (esr_pack.transpose_flip); conv5 of an RDB additionally folds the x4->x2 identity path
    (block.py:266) into its x2 output slice, and the upconvs get the 4x4/stride-2 adjoint kernel."""

    def __init__(self, convs, dtype, device, special, gathers=(), folds=()):
        # convs: list of (key, weight_param); special: key -> dict(sum=(dst,src,count)) / dict(ups=True)
        # folds: keys of nearest-x3 up-convs: the transposed operand of their folded form (9 cout -> cin) as key + '#fold'
        # gathers: gather-form operands of a dense block (include/esrgan_hip.h: esr_pack.gather), each
        # (key, dst_cout, [(weight, src_co0, scale[, fold_co0]), ...]) — K = the pieces' forward couts, in order — or,
        # for the transposed 1x1 of the backward chain, (key, 'one_t', conv1x1.weight) — 4 KB of fragments
        # (esr_pack.one_t; fp16 only)
        dt_e = _dt(dtype)[0]
        self.convs, self.special = convs, special
        self.gathers = [g for g in gathers if g[1] != 'one_t']
        self.ones = [g for g in gathers if g[1] == 'one_t'] if dt_e == L.ESR_F16 else []
        # the dgrad conv maps fwd-Cout -> fwd-Cin
        specs = [(key, w.shape[1], w.shape[0], 4 if special.get(key, {}).get('ups') else w.shape[2]) for key, w in convs]
        specs += [(key, dst_cout, sum(pc[0].shape[0] for pc in pieces), 3) for key, dst_cout, pieces in self.gathers]
        specs += [(key, 64, 32, 1) for key, _, w in self.ones]
        folds = [(key, w, None) for key, w in convs if key in frozenset(folds)]
        specs += [(key + '#fold', w.shape[1], 9 * w.shape[0], 3) for key, w, _ in folds]
        watch = ([w for _, w in convs] + [pc[0] for _, _, pieces in self.gathers for pc in pieces]
                 + [w for _, _, w in self.ones])
        super().__init__(dtype, device, [s + (L.packed_weight_bytes(*s[1:], dt_e),) for s in specs], watch, folds)

    def ensure(self, stream, force=True, record_sig=False):
        """force=True: training nets, whose weights change every optimizer step.  force=False (a frozen eval-mode net,
        the VGG feature extractor): re-pack only when a parameter's storage or version changed."""
        super().ensure(stream, force, record_sig)

    def _packs(self):
        packs = []
        for key, dst_cout, pieces in self.gathers:
            e = self.entries[key]
            chunk0 = 0
            for pc in pieces:
                w, src_co0, scale = pc[:3]
                assert w.shape[0] % self.cpg == 0 and src_co0 + dst_cout <= w.shape[1]
                packs.append(self._pack_op(w, e.w_ptr, 3, transpose_flip=1, gather=1, dst_cout=dst_cout, dst_chunk0=chunk0,
                                           dst_nchunks=e.cin // self.cpg, src_co0=src_co0, src_ks=w.shape[2],
                                           scale=scale, fold_co0=pc[3] if len(pc) > 3 else 0))
                chunk0 += w.shape[0] // self.cpg
        for key, _, w in self.ones:
            packs.append(self._pack_op(w, self.entries[key].w_ptr, 1, one_t=1, scale=1.0))
        for key, w in self.convs:
            sp = self.special.get(key, {})
            pk = self._pack_op(w, self.entries[key].w_ptr, self.entries[key].ks,
                               transpose_flip=2 if sp.get('ts2') else 1, ups_dgrad=1 if sp.get('ups') else 0)
            if 'sum' in sp:
                pk.sum_dst, pk.sum_src, pk.sum_count = sp['sum']
            packs.append(pk)
        for key, (w, b, wf, bf) in self.folded.items():
            packs.append(self._pack_op(wf, self.entries[key + '#fold'].w_ptr, 3, transpose_flip=1))
        return packs


# Unit order of a dense block's fused weight stream.  THE one place on the Python side that has to follow the kernels'
# schedule (Sched in csrc/rdb_chain_kernel.h; include/esrgan_hip.h: esr_rdb_block.w and "Backward weight stream").
#   slices:     entry suffixes of the five slice operands = cout blocks 0..3 and 4/5 of the stream
#   one:        entry suffix of the 1x1 operand
#   split:      True  — phase p < 5 is crit_p (cout block p-1 alone, one unit per K step: 3 kw x 3 kh) and then bulk_p
#                       (cout blocks p..5, one unit per (K step, kw)), so that the epilogue and halo hand-off of conv_p
#                       overlap the remaining convs; phase 5 = blocks 4/5
#               False — one unit per (K step, kw) over cout blocks p-1..5 in every phase
#   one_behind: ('crit' | 'bulk', p): the 1x1's fragments follow that unit group; None: the end of the stream
StreamLayout = collections.namedtuple('StreamLayout', 'slices one split one_behind')
_FWD_SLICES = tuple('.conv%d.0' % k for k in range(1, 6))                # conv1..conv4, conv5[0:32] / conv5[32:64]
FWD_F16 = StreamLayout(_FWD_SLICES, '.conv1x1', True, ('bulk', 1))
FWD_F32 = StreamLayout(_FWD_SLICES, '.conv1x1', False, None)
# backward (esr_rdb_backward): the gather-form operands of the x4, x3, x2, x1 slices and the x slice's two cout blocks
# in the forward's crit / bulk order, the transposed 1x1 (esr_pack.one_t) behind crit_3
BWD_F16 = StreamLayout(('.g4', '.g3', '.c2', '.g1', '.c0'), '.o1', True, ('crit', 3))


def rdb_stream_offsets(cpg, slices, one, layout):
    """Byte offsets (in the source arena) of one block's 1 KB fragments in stream order.  slices: byte offset of each
    of the five slice operands; one: byte offsets of the 1x1's fragments.  Plain integers in, plain integers out."""
    kx, kd = 64 // cpg, 32 // cpg
    nch = [(64 + 32 * k) // cpg for k in range(5)]               # K chunks of the five slice operands

    def frag(blk, c, kh, kw):
        k, cb = (blk, 0) if blk < 4 else (4, blk - 4)
        return slices[k] + (((cb * nch[k] + c) * 3 + kh) * 3 + kw) * 1024

    def bulk(first, chunks):
        return [frag(blk, c, kh, kw) for c in chunks for kw in range(3) for blk in range(first, 6) for kh in range(3)]
    offs = []
    for ph in range(1, 6):                                       # phase = input slice x, x1..x4
        c0 = 0 if ph == 1 else kx + (ph - 2) * kd
        chunks = range(c0, c0 + (kx if ph == 1 else kd))
        if layout.split and ph < 5:
            offs += [frag(ph - 1, c, kh, kw) for c in chunks for kw in range(3) for kh in range(3)]
            if layout.one_behind == ('crit', ph):
                offs += one
            offs += bulk(ph, chunks)
            if layout.one_behind == ('bulk', ph):
                offs += one
        else:
            offs += bulk(ph - 1, chunks)
    if layout.one_behind is None:
        offs += one
    return offs


class RdbWeightStreams:
    """Fused weight streams of dense blocks for the chain kernels: per block (`prefixes`) the 1 KB MFMA fragments of
    its operands in `pack` in the order the kernel's units consume them (`layout`) — a pure gather of fragments out
    of the pack's arena, run as ONE esr_gather_fragments launch after every re-pack.  Where the pack has biases, the
    biases of a block are gathered as one [192] fp32 vector as well."""

    def __init__(self, pack, prefixes, layout):
        self.pack, self.prefixes, self.layout = pack, list(prefixes), layout
        self.cpg = pack.cpg
        dev = pack.arena.device
        self.stream_bytes = L.lib().esr_rdb_weight_stream_bytes(pack.esr_dtype)
        self.arena = torch.zeros(len(self.prefixes) * self.stream_bytes, dtype=torch.uint8, device=dev)
        self.bias = None
        if pack.entries[self.prefixes[0] + layout.slices[0]].has_bias:
            self.bias = torch.zeros(len(self.prefixes) * 192, dtype=torch.float32, device=dev)   # [block][192]
        self._gen = None
        self.ops = None

    def w_ptr(self, i):
        return self.arena.data_ptr() + i * self.stream_bytes

    def bias_ptr(self, i):
        return self.bias.data_ptr() + i * 192 * 4

    def _table(self):
        ent, base, offs = self.pack.entries, self.pack.arena.data_ptr(), []
        for p in self.prefixes:
            e1 = ent[p + self.layout.one]
            n1 = L.packed_weight_bytes(e1.cout, e1.cin, e1.ks, self.pack.esr_dtype) // 1024
            offs += rdb_stream_offsets(self.cpg, [ent[p + s].w_ptr - base for s in self.layout.slices],
                                       [e1.w_ptr - base + f * 1024 for f in range(n1)], self.layout)
        assert len(offs) * 1024 == len(self.prefixes) * self.stream_bytes, (len(offs), self.stream_bytes)
        return offs

    def _gather(self, offsets, src_base, dst, piece_bytes=None):
        tab = torch.tensor(offsets, dtype=torch.int64, device=self.arena.device)
        g = L.esr_frag_gather()
        g.src_off, g.src_base, g.dst, g.n = tab.data_ptr(), src_base, dst.data_ptr(), tab.numel()
        if piece_bytes:
            g.piece_bytes = piece_bytes
        self.ops.add(L.OP_FRAG_GATHER, 'frag_gather', g)
        return tab

    def ensure(self, stream, force=False):
        """Call after pack.ensure(): re-gathers when the packed arena was rewritten."""
        if self.ops is None:
            self.ops = L.OpList()
            self._tab = self._gather(self._table(), self.pack.arena.data_ptr(), self.arena)
            if self.bias is not None:
                # the biases of a block as one [192] vector: 128-byte pieces straight from the nn.Parameters
                boffs = [self.pack.entries[p + s].bias_ptr + 128 * q
                         for p in self.prefixes for k, s in enumerate(self.layout.slices) for q in range(2 if k == 4 else 1)]
                self._btab = self._gather(boffs, None, self.bias, 128)
        gen = (self.pack.generation, self.pack.pack_count)
        if force or gen != self._gen:
            self.ops.run(stream)
            self._gen = gen


def RdbStreams(wp, prefixes):
    """Forward streams (esr_rdb_forward) over a WeightPack."""
    return RdbWeightStreams(wp, prefixes, FWD_F16 if wp.esr_dtype == L.ESR_F16 else FWD_F32)


def RdbBwdStreams(dp, prefixes):
    """Backward streams (esr_rdb_backward; fp16 only) over a DgradPack."""
    assert dp.esr_dtype == L.ESR_F16
    return RdbWeightStreams(dp, prefixes, BWD_F16)
