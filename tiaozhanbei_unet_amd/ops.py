"""autograd operators over the C-ABI of libunet_hip.so.

PyTorch is plumbing here: it owns device memory (the caching allocator), the stream and
the autograd tape; every FLOP of these operators runs in hand-written gfx950 HIP kernels
reached through ``_lib`` (ctypes).  Tensors between operators are logical-NCHW torch
tensors with ``channels_last`` strides (i.e. NHWC in memory) in the compute dtype
(``torch.bfloat16`` or ``torch.float32``).  There is no fallback: CPU tensors raise.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib as L

_DT = {torch.float32: L.UNET_F32, torch.bfloat16: L.UNET_BF16}
BN_EPS = 1e-5


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "tiaozhanbei_unet_amd runs only on an AMD GPU through libunet_hip.so; got a "
                f"{t.device} tensor (there is deliberately no CPU fallback)")


def _nhwc_empty(n, c, h, w, dtype, device):
    return torch.empty((n, c, h, w), dtype=dtype, device=device, memory_format=torch.channels_last)


def _is_nhwc(t: torch.Tensor) -> bool:
    """Dense NHWC in memory (strides of size-1 dims are irrelevant)."""
    n, c, h, w = t.shape
    want = (h * w * c, 1, w * c, c)
    return all(sz == 1 or st == wt for sz, st, wt in zip(t.shape, t.stride(), want))


def _as_nhwc(t: torch.Tensor, dtype) -> torch.Tensor:
    """Activation/gradient in the operators' layout.  (Only reached for tensors produced outside
    these operators, e.g. a test's upstream gradient.)"""
    if t.dtype == dtype and _is_nhwc(t):
        return t
    out = _nhwc_empty(*t.shape, dtype, t.device)
    out.copy_(t)
    return out


_workspaces = {}

# Data parallelism (ddp.GradientExchange) registers, per parameter, the slice of its flat all-reduce bucket: the
# weight-gradient kernels then write the gradient THERE (autograd adopts the returned tensor as ``param.grad`` when
# the parameter has no gradient yet), so no per-tensor copy into the bucket exists.
_grad_slots = {}           # parameter data_ptr -> (bucket view shaped like the parameter, weakref to the parameter)
_grad_taken = set()        # slots handed out in the current backward pass (a parameter used twice gets fresh memory)


def register_grad_slots(slots):
    _grad_slots.update(slots)


def unregister_grad_slots(keys):
    for k in keys:
        _grad_slots.pop(k, None)
        _grad_taken.discard(k)


def release_grad_slot(key):
    """The gradient of this parameter has been accumulated (post-accumulate hook): its slot may be handed out again."""
    _grad_taken.discard(key)


def grad_out(shape, device, key):
    """fp32 output tensor for the gradient of the parameter whose ``data_ptr()`` is ``key``: its registered bucket
    slice when the parameter holds no gradient yet (autograd then adopts the slice as ``param.grad``), else fresh memory."""
    slot = _grad_slots.get(key) if _grad_slots else None
    if slot is not None:
        view, ref = slot
        prm = ref()
        if prm is not None and prm.grad is None and key not in _grad_taken and tuple(view.shape) == tuple(shape) \
                and view.device == device:
            _grad_taken.add(key)
            return view.detach()            # a fresh alias: autograd adopts a gradient only if nobody else holds the tensor
    return torch.empty(tuple(shape), dtype=torch.float32, device=device)


def _workspace(nbytes: int, device) -> torch.Tensor:
    """Grow-only scratch arena per (device, stream): reuse is stream-ordered, so every compute stream has
    its own arena (the two decoders of AnomalyUNet run on two streams)."""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def _views(items) -> "L.View2":
    arr = L.View2()
    for i, it in enumerate(items):
        if it is None:
            arr[i] = L.View(None, 0, 0, 0, 0, 0)
        else:
            t, oy, ox = it
            arr[i] = L.View(t.data_ptr(), t.shape[1], t.shape[2], t.shape[3], oy, ox)
    return arr


def _pad64(c: int) -> int:
    return (c + 63) // 64 * 64


# ----------------------------------------------------------------------------- layout
class PackInput(torch.autograd.Function):
    """NCHW fp32 image batch -> NHWC compute dtype, channels zero-padded to a multiple of 64
    (the tensor entering ``self.inc`` at /root/reference/src/model.py:190)."""

    @staticmethod
    def forward(ctx, x, dtype):
        _require_cuda(x)
        x = x.contiguous().float()
        n, c, h, w = x.shape
        cp = _pad64(c)
        out = _nhwc_empty(n, cp, h, w, dtype, x.device)
        L.check(L.lib().unet_nchw_to_nhwc(_ptr(x), _ptr(out), n, c, h, w, cp, _DT[dtype], _stream()),
                "unet_nchw_to_nhwc")
        ctx.c = c
        return out

    @staticmethod
    def backward(ctx, g):
        n, cp, h, w = g.shape
        g = _as_nhwc(g, g.dtype)
        out = torch.empty((n, ctx.c, h, w), dtype=torch.float32, device=g.device)
        L.check(L.lib().unet_nhwc_to_nchw(_ptr(g), _ptr(out), n, ctx.c, h, w, cp, _DT[g.dtype], _stream()),
                "unet_nhwc_to_nchw")
        return out, None


def to_operator_layout(x: torch.Tensor, dtype) -> torch.Tensor:
    """Accept what a caller of the reference modules would pass (NCHW fp32, any channel count) or an
    activation already in operator layout.  The logical-shape view a narrow block returned (narrow_channels) gives
    back its padded tensor without a copy."""
    _require_cuda(x)
    if x.dim() != 4:
        raise ValueError(f"expected a 4-D NCHW tensor, got shape {tuple(x.shape)}")
    if x.shape[1] % 64:
        hit = _narrow_views.get(id(x))
        if hit is not None and hit[0]() is x and x._version == hit[2] and hit[1].dtype == dtype:
            return hit[1]
    if x.dtype == dtype and _is_nhwc(x) and x.shape[1] % 64 == 0:
        return x
    if x.shape[1] % 64 == 0 and x.dtype == dtype:
        return _ToNHWC.apply(x)
    return PackInput.apply(x, dtype)


class _ToNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return _as_nhwc(x, x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


# ----------------------------------------------------------------------------- widths that are not multiples of 64
# A layer of c channels runs as the layer of cp = pad64(c) channels: zero weight rows / columns and zero BatchNorm
# gamma / beta in the pad lanes keep every padded activation and gradient exactly 0 there.
_narrow_views = {}       # id(view) -> (weakref to the view, its padded tensor, the view's _version when made)


class _NarrowChannels(torch.autograd.Function):
    """[N, c, H, W] view of a padded [N, cp, H, W] operator-layout tensor; the backward widens the gradient back into a
    dense NHWC cp-wide buffer with zero pad lanes (unet_widen_channels)."""

    @staticmethod
    def forward(ctx, x, c):
        ctx.cp, ctx.dtype = x.shape[1], x.dtype
        return x[:, :c]

    @staticmethod
    def backward(ctx, g):
        n, c, h, w = g.shape
        if g.dtype not in _DT:
            g = g.float()
        out = _nhwc_empty(n, ctx.cp, h, w, ctx.dtype, g.device)
        strides = (C.c_int64 * 4)(*g.stride())
        L.check(L.lib().unet_widen_channels(_ptr(g), _DT[g.dtype], strides, n, c, h, w, _ptr(out), ctx.cp,
                                            _DT[ctx.dtype], _stream()), "unet_widen_channels")
        return out, None


def narrow_channels(x: torch.Tensor, c: int) -> torch.Tensor:
    """The logical-shape result of a narrow block: a view of its padded tensor ``x`` that to_operator_layout maps back
    to ``x`` (by identity, while the view is unmodified)."""
    import weakref
    v = _NarrowChannels.apply(x, c)
    key = id(v)

    def _gone(ref, k=key):
        if _narrow_views.get(k, (None,))[0] is ref:
            del _narrow_views[k]
    _narrow_views[key] = (weakref.ref(v, _gone), x, v._version)
    return v


def seg_cols(c_in: int, split: int) -> int:
    """Packed input columns of a 3x3 conv weight with c_in parameter columns under the segment map ``split`` (logical
    channels of source 0, stored pad64(split) wide; 0 = contiguous)."""
    return _pad64(split) + _pad64(c_in - split) if split else _pad64(c_in)


def seg_col(q: int, split: int, c_in: int) -> int:
    """Parameter column of packed column ``q`` under the segment map, -1 for a zero column (unet_seg_col)."""
    if split and q >= split:
        if q < _pad64(split):
            return -1
        q = q - _pad64(split) + split
    return q if q < c_in else -1


def _remap(items):
    """ONE unet_remap_batched launch.  items: (op, src, dst, rows, cols, inner, prows, pcols, split) -- fp32 contiguous
    [rows][cols][inner] <-> [prows][pcols][inner] (L.REMAP_PAD: padded dst; L.REMAP_UNPAD: logical dst)."""
    arr = (L.RemapDesc * len(items))()
    for i, (op, src, dst, rows, cols, inner, prows, pcols, split) in enumerate(items):
        arr[i] = L.RemapDesc(src.data_ptr(), dst.data_ptr(), rows, cols, inner, prows, pcols, split, op, 0)
    L.check(L.lib().unet_remap_batched(arr, len(items), _stream()), "unet_remap_batched")


def _vec_item(op, src, dst, c, cp):
    return (op, src, dst, 1, c, 1, 1, cp, 0)


class _NarrowBn:
    """cp-length copies of a narrow BatchNorm's gamma, beta, running_mean, running_var with zero pad lanes (one pad
    launch, plus ``extra`` pad items): the BatchNorm kernels then give scale = shift = 0 and dgamma = dbeta = 0 there.
    write_back() returns the running statistics a finalize updated to the module's buffers."""

    def __init__(self, gamma, beta, running_mean, running_var, cp, extra=()):
        c = gamma.shape[0]
        self.c, self.cp = c, cp
        self.buf = torch.empty((4, cp), dtype=torch.float32, device=gamma.device)
        self.stats = None if running_mean is None else (running_mean, running_var)
        items = [_vec_item(L.REMAP_PAD, gamma, self.buf[0], c, cp), _vec_item(L.REMAP_PAD, beta, self.buf[1], c, cp)]
        if self.stats is not None:
            items += [_vec_item(L.REMAP_PAD, running_mean, self.buf[2], c, cp),
                      _vec_item(L.REMAP_PAD, running_var, self.buf[3], c, cp)]
        _remap(items + list(extra))

    @property
    def params(self):
        b = self.buf
        return (b[0], b[1]) + ((b[2], b[3]) if self.stats is not None else (None, None))

    def write_back(self):
        if self.stats is not None:
            _remap([_vec_item(L.REMAP_UNPAD, self.buf[2], self.stats[0], self.c, self.cp),
                    _vec_item(L.REMAP_UNPAD, self.buf[3], self.stats[1], self.c, self.cp)])


def pack_weight(w: torch.Tensor, mode: int, rows: int, k: int, dtype, split: int = 0) -> torch.Tensor:
    taps = 9 if mode in (L.PACK_CONV_FWD, L.PACK_CONV_DGRAD) else 4
    out = torch.empty(taps * rows * k, dtype=dtype, device=w.device)
    if mode in (L.PACK_CONV_FWD, L.PACK_CONV_DGRAD):
        co, ci = w.shape[0], w.shape[1]
    else:
        ci, co = w.shape[0], w.shape[1]
    if split:
        L.check(L.lib().unet_pack_weight_seg(_ptr(w), _ptr(out), co, ci, rows, k, mode, split, _DT[dtype], _stream()),
                "unet_pack_weight_seg")
        return out
    L.check(L.lib().unet_pack_weight(_ptr(w), _ptr(out), co, ci, rows, k, mode, _DT[dtype], _stream()),
            "unet_pack_weight")
    return out


class PackCache:
    """Packed GEMM-layout copies of a model's conv / convT weights, refreshed by ONE batched launch whenever a
    parameter changed (its autograd version counter moved), instead of ~70 small pack launches per step."""

    def __init__(self, dtype):
        self.dtype = dtype
        self.items = []        # (weight, mode, rows, k, split)
        self.slots = {}        # (id(weight), mode) -> [packed view, rows, k, version, split]
        self.table = None
        self.ptrs = None
        self.gen = -1          # ops._train_generation when the packs were last written
        self.wgen = -1         # ops._write_generation then (see get)
        self.owners = []       # (model.py) where each cached weight lives in its model, to notice a replaced Parameter
        self.witnesses = []    # (model.py) the model's buffers: a moved version counter of one of them means that
        self.seen = None       # somebody rewrote the model's state (their counters at the last pack)

    def add(self, weight, mode, rows, k, split=0):
        """``split``: segment map of a 3x3 conv weight's input channels (unet_pack_desc.reserved; 0 = contiguous)."""
        if (id(weight), mode) not in self.slots:
            self.items.append((weight, mode, rows, k, split))
            self.slots[(id(weight), mode)] = [None, rows, k, -1, split]

    def _build(self):
        import numpy as np
        es = 2 if self.dtype == torch.bfloat16 else 4
        sizes = [(9 if m <= L.PACK_CONV_DGRAD else 4) * r * k for (_, m, r, k, _) in self.items]
        offs = [0]
        for s_ in sizes:
            offs.append(offs[-1] + (s_ + 7) // 8 * 8)
        dev = self.items[0][0].device
        self.buf = torch.empty(offs[-1], dtype=self.dtype, device=dev)
        rec = np.zeros(len(self.items), dtype=[("w", "<u8"), ("out", "<u8"), ("c_out", "<i4"), ("c_in", "<i4"),
                                               ("rows", "<i4"), ("k", "<i4"), ("mode", "<i4"), ("pad", "<i4")])
        for i, (w, m, r, k, sp) in enumerate(self.items):
            view = self.buf[offs[i]:offs[i] + sizes[i]]
            co, ci = (w.shape[0], w.shape[1]) if m <= L.PACK_CONV_DGRAD else (w.shape[1], w.shape[0])
            rec[i] = (w.data_ptr(), view.data_ptr(), co, ci, r, k, m, sp)
            self.slots[(id(w), m)][0] = view
        self.table = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
        self.ptrs = [w.data_ptr() for (w, _, _, _, _) in self.items]

    def refresh(self, force=False):
        """``force``: repack regardless of the version counters (fused optimisers update parameters without
        moving them, so a training forward always repacks: one ~0.1 ms launch).  An eval-mode forward repacks when
        ``_train_generation`` moved since the last pack: a fused optimiser step (``parameters_written``) changed the
        weights through raw pointers that no version counter sees -- also when every BatchNorm was frozen during the
        step, so that no layer ran a training forward.  It also repacks when a version counter of one of the model's
        BUFFERS moved: whoever rewrites a model wholesale writes those, too -- torch.optim.swa_utils.AveragedModel
        syncs or averages them in every update_parameters, while the torch._foreach_lerp_ it averages the weights with
        moves no version counter on the GPU (torch 2.10)."""
        if not self.items:
            return
        if self.table is None or self.ptrs != [w.data_ptr() for (w, _, _, _, _) in self.items]:
            self._build()
            stale = True
        else:
            stale = force or self.gen != _train_generation or \
                any(self.slots[(id(w), m)][3] != w._version for (w, m, _, _, _) in self.items) or \
                self.seen != [b._version for b in self.witnesses]
        if stale:
            L.check(L.lib().unet_pack_weights_batched(_ptr(self.table), len(self.items), _DT[self.dtype], _stream()),
                    "unet_pack_weights_batched")
            for (w, m, _, _, _) in self.items:
                self.slots[(id(w), m)][3] = w._version
            self.gen = _train_generation
            self.wgen = _write_generation
            self.seen = [b._version for b in self.witnesses]

    def get(self, weight, mode, rows, k, split=0):
        """The pack of ``weight`` if it is current: version counter unchanged and no ``parameters_written()`` since the
        last refresh (a block of the model called on its own runs no refresh; it then takes a pack of its own)."""
        s_ = self.slots.get((id(weight), mode))
        if s_ is not None and s_[0] is not None and s_[1] == rows and s_[2] == k and s_[3] == weight._version \
                and s_[4] == split and self.wgen == _write_generation:
            return s_[0]
        return None


_active_packs = None       # weak reference to the cache of the model that ran last (the model owns it: a deleted
                           # model's packs and weights go with it)


def set_active_packs(cache):
    global _active_packs
    import weakref
    _active_packs = None if cache is None else weakref.ref(cache)


def packed(weight, mode, rows, k, dtype, split=0):
    cache = _active_packs() if _active_packs is not None else None
    if cache is not None and cache.dtype == dtype:
        hit = cache.get(weight, mode, rows, k, split)
        if hit is not None:
            return hit
    return pack_weight(weight, mode, rows, k, dtype, split)


# ----------------------------------------------------------------------------- gradient fan-in of the skips
class GradSink:
    """In-place gradient fan-in of an activation with several consumers (the skip tensors x1..x4 feed the
    next encoder level and both decoders, /root/reference/src/model.py:190-207).

    Autograd would materialise one gradient per consumer and add them with two more elementwise passes
    (9 tensor sweeps per skip).  With a sink the first consumer to run its backward WRITES the buffer and
    hands it to autograd, the later ones ACCUMULATE into it inside their own kernel epilogue
    (`accumulate` of unet_conv3x3 / unet_maxpool2_bwd) and return no gradient (5 sweeps).  The order is the
    autograd engine's (deterministic for a fixed graph); writers on different HIP streams are chained by
    events, and the producer's backward waits for the last one."""

    __slots__ = ("buf", "event")

    def __init__(self):
        self.buf = None
        self.event = None

    def begin(self, dev):
        """-> True when the caller must accumulate into ``self.buf`` (someone wrote it already)."""
        if self.buf is None:
            return False
        cur = torch.cuda.current_stream(dev)
        if self.event is not None:
            cur.wait_event(self.event)
        self.buf.record_stream(cur)
        return True

    def done(self, buf, dev):
        self.buf = buf
        self.event = torch.cuda.Event()
        self.event.record(torch.cuda.current_stream(dev))

    def collect(self, grad, dev):
        """Called by the producer's backward with the gradient autograd delivered."""
        if self.buf is not None:
            if grad.data_ptr() != self.buf.data_ptr():
                raise RuntimeError("GradSink: autograd delivered a different tensor than the shared gradient buffer")
            cur = torch.cuda.current_stream(dev)
            if self.event is not None:
                cur.wait_event(self.event)
            self.buf.record_stream(cur)
        self.buf = None
        self.event = None


SHARE_SKIP_GRADS = __import__("os").environ.get("UNET_GRAD_SINK", "1") != "0"


def share_grad(t: torch.Tensor) -> torch.Tensor:
    """Mark an operator output whose gradient has several consumers (model code calls this on the skips)."""
    if SHARE_SKIP_GRADS and t.grad_fn is not None and hasattr(t.grad_fn, "out_sink"):
        sink = GradSink()
        t.grad_fn.out_sink = sink
        t._unet_sink = sink
    return t


FOLD_EVAL_BN = __import__("os").environ.get("UNET_FOLD_BN", "1") != "0"
_folded = {}                                             # id(weight) -> (weakref to it, {(dtype, ctot): (stamp, payload)})
_train_generation = 0                                    # bumped by every training forward (see below) and by
                                                         # parameters_written()
_write_generation = 0                                    # bumped by parameters_written() alone


def parameters_written():
    """To be called by whatever updates parameters (or BatchNorm buffers) through raw pointers, where no autograd version
    counter moves (optim.FusedAdam.step): every packed copy of them -- PackCache, the folded BatchNorm packs -- is stale
    from here on.  A training forward does the same for the running statistics its kernels write.  Both are host-side
    counters: an update replayed from a captured graph does not run them, so whoever replays one calls this after it.
    The same holds for any write through ``param.data`` (``p.data.copy_()``, ``m.weight.data.normal_()``): it moves no
    version counter either.  Exported as ``tiaozhanbei_unet_amd.parameters_written``."""
    global _train_generation, _write_generation
    _train_generation += 1
    _write_generation += 1


def _folded_pack(weight, gamma, beta, running_mean, running_var, co, ctot, dtype, rows=None, split=0):
    """(packed folded weights, shift) of an eval-mode conv+BN layer.  Cached per weight Parameter; an entry is valid
    while the autograd version counters of the five tensors AND the training generation are unchanged -- the HIP
    kernels update running statistics (and fused optimisers update parameters) through raw pointers, which no version
    counter sees, so any training forward or fused optimiser step (``parameters_written``) in between invalidates
    every entry.  ``rows`` (> co for a narrow layer:
    zero-padded BatchNorm coefficients, zero weight rows) and ``split`` (segment map of the input channels) give the
    padded layer's pack."""
    stamp = (_train_generation, weight._version, gamma._version, beta._version, running_mean._version,
             running_var._version, running_mean.data_ptr(), running_var.data_ptr(), weight.data_ptr())
    import weakref
    slot = _folded.get(id(weight))
    if slot is None or slot[0]() is not weight:          # first use, or the id was recycled by another tensor
        key = id(weight)
        slot = (weakref.ref(weight, lambda _r, k=key: _folded.pop(k, None)), {})
        _folded[key] = slot
    per_weight = slot[1]
    rows = co if rows is None else rows
    key = (dtype, ctot) if (rows == co and not split) else (dtype, ctot, rows, split)
    hit = per_weight.get(key)
    if hit is not None and hit[0] == stamp:
        return hit[1]
    lib, st, dev = L.lib(), _stream(), weight.device
    if key != (dtype, ctot):
        g, b, rm, rv = _NarrowBn(gamma, beta, running_mean, running_var, rows).params
        ss = torch.empty((2, rows), dtype=torch.float32, device=dev)
        L.check(lib.unet_bn_eval_coeffs(rows, _ptr(g), _ptr(b), _ptr(rm), _ptr(rv), BN_EPS, _ptr(ss[0]), _ptr(ss[1]), st),
                "unet_bn_eval_coeffs")
        wq = torch.empty(9 * rows * ctot, dtype=dtype, device=dev)
        L.check(lib.unet_pack_conv_weight_folded_seg(_ptr(weight.detach()), _ptr(ss[0]), _ptr(wq), co, weight.shape[1],
                                                     rows, ctot, split, _DT[dtype], st), "unet_pack_conv_weight_folded_seg")
        per_weight[key] = (stamp, (wq, ss[1]))
        return wq, ss[1]
    ss = torch.empty((2, co), dtype=torch.float32, device=dev)
    L.check(lib.unet_bn_eval_coeffs(co, _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), BN_EPS,
                                    _ptr(ss[0]), _ptr(ss[1]), st), "unet_bn_eval_coeffs")
    wq = torch.empty(9 * co * ctot, dtype=dtype, device=dev)
    L.check(lib.unet_pack_conv_weight_folded(_ptr(weight.detach()), _ptr(ss[0]), _ptr(wq), co, weight.shape[1], co, ctot,
                                             _DT[dtype], st), "unet_pack_conv_weight_folded")
    per_weight[(dtype, ctot)] = (stamp, (wq, ss[1]))
    return wq, ss[1]


# ----------------------------------------------------------------------------- conv3x3 + BN + ReLU
FUSE_BN_BWD = __import__("os").environ.get("UNET_FUSE_BN_BWD", "1") != "0"      # tuning hook (A/B runs)
FUSE_BN_HEAD = __import__("os").environ.get("UNET_FUSE_BN_HEAD", "1") != "0"
FUSE_BN_POOL = __import__("os").environ.get("UNET_FUSE_BN_POOL", "1") != "0"
FUSE_BN_CONVT = __import__("os").environ.get("UNET_FUSE_BN_CONVT", "1") != "0"


class BnLink:
    """Side channel between a conv-BN-ReLU layer and the ONE operator that consumes its activation (the second
    convolution of the same DoubleConv, /root/reference/src/model.py:14-19).  In the backward pass the consumer's data
    gradient kernel applies this layer's ReLU mask in its epilogue and leaves the BatchNorm-backward partial sums
    (sum dz, sum dz*(y - mean)) here, so the producer skips its reduction pass over (y, da).  Only valid for an
    activation with exactly one consumer -- the model code creates links for DoubleConv's internal tensor only."""

    __slots__ = ("y", "coef", "partial", "n_parts", "dz_ptr")

    def __init__(self):
        self.y = None          # raw conv output of the producer (NHWC compute dtype)
        self.coef = None       # [4, C]: mean, istd, scale, shift
        self.partial = None
        self.n_parts = 0
        self.dz_ptr = 0        # data_ptr of the premasked gradient the consumer returned (0: not premasked)


def _bn_stats_conv(lib, dt, n, h, w, src, wp, co, y, gamma, beta, running_mean, running_var, momentum, coef, dev, st):
    """conv + BatchNorm batch statistics in one call (the conv epilogue reduces sum / sum of squares per channel
    with wavefront shuffles, or one extra streaming pass for kernels without that epilogue) + fp64 finalize."""
    cap = lib.unet_conv3x3_stats_max_parts(n, h, w)
    part = _workspace(cap * 2 * co * 4, dev)
    nparts = C.c_int32(0)
    L.check(lib.unet_conv3x3_stats(dt, n, h, w, src, _ptr(wp), co, _ptr(y), _ptr(part), C.byref(nparts), st),
            "unet_conv3x3_stats")
    L.check(lib.unet_bn_finalize_partials(_ptr(part), nparts.value, n * h * w, co, _ptr(gamma), _ptr(beta),
                                          _ptr(running_mean), _ptr(running_var), momentum, BN_EPS,
                                          _ptr(coef[0]), _ptr(coef[1]), _ptr(coef[2]), _ptr(coef[3]), st),
            "unet_bn_finalize_partials")


def _bn_relu_backward(lib, dt, dtype, da, y, gamma, coef, link, out_sink, dev, st, frozen=False, beta_key=None,
                      gamma_key=None):
    """Gradient w.r.t. the raw conv output of a conv-BN-ReLU layer -> (dy, dgamma/dbeta [2, C]).  Premasked path: the
    consumer's data-gradient kernel already applied the ReLU mask and reduced the BatchNorm-backward sums (BnLink).
    ``frozen``: the layer normalised with its running statistics (BatchNorm2d in eval mode inside a training graph)."""
    n, co, h, w = y.shape
    pixels = n * h * w
    dgb = (grad_out(gamma.shape, dev, gamma.data_ptr() if gamma_key is None else gamma_key),
           grad_out(gamma.shape, dev, beta_key))
    if link is not None and link.dz_ptr and link.dz_ptr == da.data_ptr() and da.dtype == dtype and _is_nhwc(da):
        dy = da
        ws = _workspace(3 * co * 4, dev)
        L.check(lib.unet_bn_bwd_premasked(dt, _ptr(da), _ptr(y), pixels, co, _ptr(gamma), _ptr(coef[0]),
                                          _ptr(coef[1]), _ptr(link.partial), link.n_parts, _ptr(dgb[0]),
                                          _ptr(dgb[1]), _ptr(dy), _ptr(ws), ws.numel(), st), "unet_bn_bwd_premasked")
    else:
        if link is not None and link.dz_ptr:
            raise RuntimeError("conv-BN-ReLU: the premasked gradient of a linked activation did not arrive unchanged "
                               "(the activation has a second consumer?)")
        if out_sink is not None:
            out_sink.collect(da, dev)
        da = _as_nhwc(da, dtype)
        dy = _nhwc_empty(n, co, h, w, dtype, dev)
        ws = _workspace(lib.unet_bn_workspace(pixels, co), dev)
        fn = lib.unet_bn_relu_bwd_frozen if frozen else lib.unet_bn_relu_bwd
        L.check(fn(dt, _ptr(da), _ptr(y), pixels, co, _ptr(gamma), _ptr(coef[0]), _ptr(coef[1]),
                   _ptr(coef[2]), _ptr(coef[3]), _ptr(dgb[0]), _ptr(dgb[1]), _ptr(dy),
                   _ptr(ws), ws.numel(), st), "unet_bn_relu_bwd")
    if link is not None:
        link.y = link.coef = link.partial = None
        link.dz_ptr = 0
    return dy, dgb


class ConvBnRelu(torch.autograd.Function):
    """relu(batch_norm(conv3x3(cat([x0, x1])))) -- one third of DoubleConv
    (/root/reference/src/model.py:14-16 / :17-19); ``x1`` (optional) is the up-sampled tensor
    of Up.forward, centre-padded to x0's size (src/model.py:57-65) without materialising pad or cat.

    Optional fusions of the training path (all value-preserving):
      * ``head_w`` / ``head_b`` / ``head_sigmoid``: the layer is followed by OutConv (src/model.py:72): the 1x1 head
        reads the RAW conv output and applies BatchNorm + ReLU on load, its backward writes the ReLU-masked gradient
        and the BatchNorm-backward sums -- no activation tensor, no BN-apply pass, no (y, da) reduction pass.
        The function then returns the head's NCHW fp32 output.
      * ``out_link`` / ``in_link`` (BnLink): see BnLink.
      * ``pool``: the layer closes an encoder level (src/model.py:18-19, next level's MaxPool2d :32): BatchNorm-apply +
        ReLU + 2x2 max pool in one pass; returns (a, maxpool2(a)).  The backward routes the pooled gradient, adds it to
        what the decoders left in the skip's gradient buffer, masks and reduces in one pass (no separate pool backward,
        no (y, da) reduction pass).

    Widths: a layer whose output channel count is not a multiple of 64 runs as the padded layer (zero weight rows,
    zero-padded BatchNorm parameters, running statistics written back) and returns padded tensors; ``split`` = logical
    channels of a narrow ``x0`` next to ``x1`` (the segment map of the packed input channels, 0 = contiguous)."""

    @staticmethod
    def forward(ctx, x0, x1, weight, gamma, beta, running_mean, running_var, training, momentum, fold=False,
                in_link=None, out_link=None, head_w=None, head_b=None, head_sigmoid=False, pool=False, split=0):
        _require_cuda(x0, weight)
        dtype = x0.dtype
        dt = _DT[dtype]
        n, c0, h, w = x0.shape
        c1 = 0 if x1 is None else x1.shape[1]
        oy = ox = 0
        if x1 is not None:
            dy_, dx_ = h - x1.shape[2], w - x1.shape[3]
            if dy_ < 0 or dx_ < 0:
                raise ValueError("Up: the skip tensor must be at least as large as the up-sampled one")
            oy, ox = dy_ // 2, dx_ // 2
        co_p, ci = weight.shape[0], weight.shape[1]
        co = _pad64(co_p)                     # the kernels' output width (co_p itself for multiples of 64)
        ctot = c0 + c1
        split = int(split or 0)
        if split:
            if x1 is None or c0 != _pad64(split) or ctot != seg_cols(ci, split):
                raise ValueError(f"conv weight expects {split} + {ci - split} input channels, activations carry "
                                 f"{c0} + {c1} (padded)")
        elif not (ci <= ctot < ci + 64):
            raise ValueError(f"conv weight expects {ci} input channels, activations carry {ctot}")
        if (head_w is not None or pool) and not training:
            raise RuntimeError("ConvBnRelu: the fused head / pool are training-path fusions")
        lib, st, dev = L.lib(), _stream(), x0.device
        bn_param = (gamma, beta, running_mean, running_var)
        narrow = co != co_p
        y = _nhwc_empty(n, co, h, w, dtype, dev)
        src = _views([(x0, 0, 0), None if x1 is None else (x1, oy, ox)])
        pixels = n * h * w
        coef = torch.empty((4, co), dtype=torch.float32, device=dev)   # mean, istd, scale, shift
        fold = bool(fold) and FOLD_EVAL_BN and not training
        nb = None
        if not fold:
            wp = packed(weight, L.PACK_CONV_FWD, co, ctot, dtype, split)
            if narrow:
                nb = _NarrowBn(gamma, beta, running_mean, running_var, co)
                gamma, beta, running_mean, running_var = nb.params
        if training:
            global _train_generation
            _train_generation += 1
            _bn_stats_conv(lib, dt, n, h, w, src, wp, co, y, gamma, beta, running_mean, running_var, momentum, coef,
                           dev, st)
            if nb is not None:
                nb.write_back()
        elif fold:
            # inference: BatchNorm(eval) folded into the layer -- scale into the packed weights, shift + ReLU in the
            # convolution's epilogue: one kernel, the activation is written once
            if narrow or split:
                wf = _folded_pack(weight, *bn_param, co_p, ctot, dtype, rows=co, split=split)
            else:
                wf = _folded_pack(weight, gamma, beta, running_mean, running_var, co, ctot, dtype)
            L.check(lib.unet_conv3x3_bias_relu(dt, n, h, w, src, _ptr(wf[0]), co, _ptr(y), _ptr(wf[1]), 1, st),
                    "unet_conv3x3_bias_relu")
            return y
        else:
            dst = _views([(y, 0, 0), None])
            L.check(lib.unet_conv3x3(dt, n, h, w, src, _ptr(wp), co, dst, co, 0, L.K_CONV_FWD, st), "unet_conv3x3")
            L.check(lib.unet_bn_eval_coeffs4(co, _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var),
                                             BN_EPS, _ptr(coef[0]), _ptr(coef[1]), _ptr(coef[2]), _ptr(coef[3]), st),
                    "unet_bn_eval_coeffs4")
        ctx.geom = (oy, ox, training)
        ctx.keys = (weight.data_ptr(), bn_param[1].data_ptr(), 0 if head_w is None else head_w.data_ptr(),
                    0 if head_b is None else head_b.data_ptr())          # gradient bucket slots (data parallelism)
        ctx.widths = (co_p, split, bn_param[0].data_ptr())
        ctx.sink0 = getattr(x0, "_unet_sink", None)     # x0 is a skip with a shared gradient buffer
        ctx.out_sink = None                              # set by share_grad() when THIS output is a skip
        ctx.in_link = in_link if (in_link is not None and in_link.y is not None and x1 is None) else None
        ctx.out_link = None
        ctx.head = None
        ctx.pool = False
        if pool:
            a = _nhwc_empty(n, co, h, w, dtype, dev)
            pooled = _nhwc_empty(n, co, h // 2, w // 2, dtype, dev)
            L.check(lib.unet_bn_relu_pool_fwd(dt, _ptr(y), n, h, w, co, _ptr(coef[2]), _ptr(coef[3]), _ptr(a),
                                              _ptr(pooled), st), "unet_bn_relu_pool_fwd")
            ctx.save_for_backward(x0, x1, y, weight, gamma, coef)
            ctx.pool = True
            ctx.set_materialize_grads(False)
            return a, pooled
        if head_w is not None:
            hc = head_w.shape[0]
            if narrow:                        # head weight [hc][co_p] -> [hc][co], zero columns
                hw_p = torch.empty((hc, co, 1, 1), dtype=torch.float32, device=dev)
                _remap([(L.REMAP_PAD, head_w.detach(), hw_p, hc, co_p, 1, hc, co, 0)])
                head_w = hw_p
            out = torch.empty((n, hc, h, w), dtype=torch.float32, device=dev)
            L.check(lib.unet_head_bnrelu_fwd(dt, _ptr(y), n, h, w, co, _ptr(coef[2]), _ptr(coef[3]), _ptr(head_w),
                                             _ptr(head_b), hc, int(head_sigmoid), _ptr(out), st), "unet_head_bnrelu_fwd")
            ctx.save_for_backward(x0, x1, y, weight, gamma, coef, head_w, out)
            ctx.head = bool(head_sigmoid)
            return out
        a = _nhwc_empty(n, co, h, w, dtype, dev)
        L.check(lib.unet_bn_relu_apply(dt, _ptr(y), pixels, co, _ptr(coef[2]), _ptr(coef[3]), _ptr(a), st),
                "unet_bn_relu_apply")
        ctx.save_for_backward(x0, x1, y, weight, gamma, coef)
        if out_link is not None and training:
            out_link.y, out_link.coef, out_link.dz_ptr = y, coef, 0
            ctx.out_link = out_link
        return a

    @staticmethod
    def backward(ctx, da, dpooled=None):
        saved = ctx.saved_tensors
        x0, x1, y, weight, gamma, coef = saved[:6]
        oy, ox, training = ctx.geom
        dtype = x0.dtype
        dt = _DT[dtype]
        n, c0, h, w = x0.shape
        co, ci = y.shape[1], weight.shape[1]
        co_p, split, gamma_key = ctx.widths
        narrow = co != co_p
        # a narrow layer's gradients w.r.t. gamma / beta / the head weight come out padded: fresh memory, unpadded last
        gkey, bkey, hkey = (0, 0, 0) if narrow else (gamma_key, ctx.keys[1], ctx.keys[2])
        ctot = c0 + (0 if x1 is None else x1.shape[1])
        lib, st, dev = L.lib(), _stream(), x0.device
        pixels = n * h * w
        dhw = dhb = None
        link = ctx.out_link
        if ctx.head is not None:
            # OutConv backward + ReLU mask + BatchNorm-backward sums in one pass that stores no dz, the coefficients, then
            # dy = A*dz + B*y + K written once with dz formed again from dout and the filters
            head_w, out = saved[6], saved[7]
            hc = head_w.shape[0]
            dout = da.contiguous().float()
            dy = _nhwc_empty(n, co, h, w, dtype, dev)
            dgb = (grad_out(gamma.shape, dev, gkey), grad_out(gamma.shape, dev, bkey))
            dhw = grad_out(head_w.shape, dev, hkey)
            dhb = grad_out((hc,), dev, ctx.keys[3])
            part = torch.empty((lib.unet_head_bnrelu_max_parts(), 2, co), dtype=torch.float32, device=dev)
            nparts = C.c_int32(0)
            ws = _workspace(lib.unet_head_bwd_workspace(n, h, w, co, hc), dev)
            L.check(lib.unet_head_bnrelu_bwd_sums(dt, _ptr(y), _ptr(coef[2]), _ptr(coef[3]), _ptr(coef[0]), _ptr(out),
                                                  _ptr(dout), n, h, w, co, _ptr(head_w), hc, int(ctx.head), _ptr(dhw),
                                                  _ptr(dhb), _ptr(part), C.byref(nparts), _ptr(ws), ws.numel(), st),
                    "unet_head_bnrelu_bwd_sums")
            cf = _workspace(3 * co * 4, dev)
            L.check(lib.unet_bn_bwd_premasked(dt, None, None, pixels, co, _ptr(gamma), _ptr(coef[0]), _ptr(coef[1]),
                                              _ptr(part), nparts.value, _ptr(dgb[0]), _ptr(dgb[1]), None, _ptr(cf),
                                              cf.numel(), st), "unet_bn_bwd_premasked(coefficients)")
            L.check(lib.unet_head_bnrelu_bwd_apply(dt, _ptr(y), _ptr(coef[2]), _ptr(coef[3]), _ptr(out), _ptr(dout), n, h,
                                                   w, co, _ptr(head_w), hc, int(ctx.head), _ptr(cf), _ptr(dy), st),
                    "unet_head_bnrelu_bwd_apply")
        elif ctx.pool and dpooled is not None:
            # pooled gradient routed + added to the skip's gradient buffer + ReLU mask + BatchNorm-backward sums: one pass
            # that stores nothing, the coefficients, then the same routing again with dy = A*dz + B*y + K written once
            own = False            # `da` is the GradSink buffer of this skip: nobody else holds it, safe to overwrite
            if da is not None:
                if ctx.out_sink is not None and ctx.out_sink.buf is not None and \
                        da.data_ptr() == ctx.out_sink.buf.data_ptr():
                    own = True
                if ctx.out_sink is not None:
                    ctx.out_sink.collect(da, dev)
                da = _as_nhwc(da, dtype)
            dpooled = _as_nhwc(dpooled, dtype)
            # in place over the skip's own gradient buffer; a gradient autograd delivered from elsewhere may be shared
            # with another node (e.g. add-backward hands one tensor to both inputs) and is left untouched
            dy = da if own else _nhwc_empty(n, co, h, w, dtype, dev)
            part = torch.empty((lib.unet_bn_relu_pool_max_parts(), 2, co), dtype=torch.float32, device=dev)
            nparts = C.c_int32(0)
            L.check(lib.unet_bn_relu_pool_bwd_sums(dt, _ptr(y), _ptr(dpooled), _ptr(da), n, h, w, co, _ptr(coef[2]),
                                                   _ptr(coef[3]), _ptr(coef[0]), _ptr(part), C.byref(nparts), st),
                    "unet_bn_relu_pool_bwd_sums")
            dgb = (grad_out(gamma.shape, dev, gkey), grad_out(gamma.shape, dev, bkey))
            cf = _workspace(3 * co * 4, dev)
            L.check(lib.unet_bn_bwd_premasked(dt, None, None, pixels, co, _ptr(gamma), _ptr(coef[0]), _ptr(coef[1]),
                                              _ptr(part), nparts.value, _ptr(dgb[0]), _ptr(dgb[1]), None, _ptr(cf),
                                              cf.numel(), st), "unet_bn_bwd_premasked(coefficients)")
            L.check(lib.unet_bn_relu_pool_bwd_apply(dt, _ptr(y), _ptr(dpooled), _ptr(da), n, h, w, co, _ptr(coef[2]),
                                                    _ptr(coef[3]), _ptr(cf), _ptr(dy), st), "unet_bn_relu_pool_bwd_apply")
        else:
            if da is None:                       # (a pooled pair whose skip half nobody used, and no pooled gradient)
                da = torch.zeros_like(y)
            dy, dgb = _bn_relu_backward(lib, dt, dtype, da, y, gamma, coef, link, ctx.out_sink, dev, st,
                                        frozen=not training, beta_key=bkey, gamma_key=gkey)
        src = _views([(x0, 0, 0), None if x1 is None else (x1, oy, ox)])
        dw = None
        if ctx.needs_input_grad[2]:
            # padded layer: the kernel writes dW of the padded one ([co][ctot] under a segment map, [co][ci] else)
            ci_k = ctot if split else ci
            dw = torch.empty((co, ci_k, 3, 3), dtype=torch.float32, device=dev) if (narrow or split) else \
                grad_out(weight.shape, dev, ctx.keys[0])
            need = lib.unet_conv3x3_wgrad_workspace(n, h, w, ctot, co)
            ws2 = _workspace(need, dev)
            L.check(lib.unet_conv3x3_wgrad(dt, n, h, w, src, _ptr(dy), co, _ptr(dw), ci_k, _ptr(ws2), ws2.numel(), st),
                    "unet_conv3x3_wgrad")
        dx0 = dx1 = None
        if ctx.needs_input_grad[0] or (x1 is not None and ctx.needs_input_grad[1]):
            wp = packed(weight, L.PACK_CONV_DGRAD, ctot, co, dtype, split)
            sink = ctx.sink0
            ilink = ctx.in_link if (FUSE_BN_BWD and sink is None and x1 is None) else None
            if ilink is not None and ilink.y is not None and \
                    lib.unet_conv3x3_dgrad_bnrelu_supported(dt, n, h, w, co, c0):
                # data gradient + ReLU mask of the PRODUCER of x0 + its BatchNorm-backward sums in one kernel
                dx0 = _nhwc_empty(n, c0, h, w, dtype, dev)
                cap = lib.unet_conv3x3_stats_max_parts(n, h, w)
                part = torch.empty((cap, 2, c0), dtype=torch.float32, device=dev)
                nparts = C.c_int32(0)
                pc = ilink.coef
                L.check(lib.unet_conv3x3_dgrad_bnrelu(dt, n, h, w, _ptr(dy), co, _ptr(wp), c0, _ptr(ilink.y),
                                                      _ptr(pc[2]), _ptr(pc[3]), _ptr(pc[0]), _ptr(dx0), _ptr(part),
                                                      C.byref(nparts), st), "unet_conv3x3_dgrad_bnrelu")
                ilink.partial, ilink.n_parts, ilink.dz_ptr = part, nparts.value, dx0.data_ptr()
            else:
                fan_in = sink is not None and sink.begin(dev)
                dx0 = sink.buf if fan_in else _nhwc_empty(n, c0, h, w, dtype, dev)
                if x1 is not None:
                    dx1 = _nhwc_empty(*x1.shape, dtype, dev)
                dsrc = _views([(dy, 0, 0), None])
                ddst = _views([(dx0, 0, 0), None if x1 is None else (dx1, oy, ox)])
                L.check(lib.unet_conv3x3(dt, n, h, w, dsrc, _ptr(wp), ctot, ddst, c0, 1 if fan_in else 0,
                                         L.K_CONV_DGRAD, st), "unet_conv3x3(dgrad)")
                if sink is not None:
                    sink.done(dx0, dev)
                    if fan_in:
                        dx0 = None              # already inside the buffer the first consumer returned
        if narrow or split:
            # padded gradients -> the parameters' shapes, one launch
            items = []
            if dw is not None:
                dw, dw_pad = grad_out(weight.shape, dev, ctx.keys[0]), dw
                items.append((L.REMAP_UNPAD, dw_pad, dw, co_p, ci, 9, co, dw_pad.shape[1], split))
            if narrow:
                dgb_pad, dgb = dgb, (grad_out((co_p,), dev, gamma_key), grad_out((co_p,), dev, ctx.keys[1]))
                items += [_vec_item(L.REMAP_UNPAD, dgb_pad[0], dgb[0], co_p, co),
                          _vec_item(L.REMAP_UNPAD, dgb_pad[1], dgb[1], co_p, co)]
                if dhw is not None:
                    hc = dhw.shape[0]
                    dhw, dhw_pad = grad_out((hc, co_p, 1, 1), dev, ctx.keys[2]), dhw
                    items.append((L.REMAP_UNPAD, dhw_pad, dhw, hc, co_p, 1, hc, co, 0))
            if items:
                _remap(items)
        return dx0, dx1, dw, dgb[0], dgb[1], None, None, None, None, None, None, None, dhw, dhb, None, None, None


class FirstConvBnRelu(torch.autograd.Function):
    """relu(batch_norm(conv3x3(image))) for the first layer of the network (inc.double_conv.0..2,
    /root/reference/src/model.py:14-16) in bf16 mode, straight from the caller's fp32 NCHW image: with 9*Cin <= 32
    the reduction is one MFMA step (unet_conv3x3_first_*), no 64-channel padded copy of the image exists."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, running_mean, running_var, training, momentum, out_link=None):
        _require_cuda(x, weight)
        x = x.contiguous().float()
        n, ci, h, w = x.shape
        co_p = weight.shape[0]
        co = _pad64(co_p)                     # 64: a narrow image layer runs with zero weight rows
        dtype = torch.bfloat16
        lib, st, dev = L.lib(), _stream(), x.device
        y = _nhwc_empty(n, co, h, w, dtype, dev)
        pixels = n * h * w
        coef = torch.empty((4, co), dtype=torch.float32, device=dev)
        wq = weight.detach().contiguous()
        ctx.keys = (weight.data_ptr(), beta.data_ptr(), gamma.data_ptr())
        nb = None
        if co != co_p:
            wq_p = torch.empty((co, ci, 3, 3), dtype=torch.float32, device=dev)
            nb = _NarrowBn(gamma, beta, running_mean, running_var, co,
                           extra=[(L.REMAP_PAD, wq, wq_p, co_p, ci, 9, co, ci, 0)])
            wq = wq_p
            gamma, beta, running_mean, running_var = nb.params
        if training:
            cap = lib.unet_conv3x3_stats_max_parts(n, h, w)
            part = _workspace(cap * 2 * co * 4, dev)
            nparts = C.c_int32(0)
            L.check(lib.unet_conv3x3_first_stats(n, h, w, _ptr(x), ci, _ptr(wq), _ptr(y), _ptr(part), C.byref(nparts), st),
                    "unet_conv3x3_first_stats")
            L.check(lib.unet_bn_finalize_partials(_ptr(part), nparts.value, pixels, co, _ptr(gamma), _ptr(beta),
                                                  _ptr(running_mean), _ptr(running_var), momentum, BN_EPS,
                                                  _ptr(coef[0]), _ptr(coef[1]), _ptr(coef[2]), _ptr(coef[3]), st),
                    "unet_bn_finalize_partials")
            if nb is not None:
                nb.write_back()
        else:
            L.check(lib.unet_conv3x3_first_stats(n, h, w, _ptr(x), ci, _ptr(wq), _ptr(y), None, None, st),
                    "unet_conv3x3_first_stats")
            L.check(lib.unet_bn_eval_coeffs4(co, _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var),
                                             BN_EPS, _ptr(coef[0]), _ptr(coef[1]), _ptr(coef[2]), _ptr(coef[3]), st),
                    "unet_bn_eval_coeffs4")
        a = _nhwc_empty(n, co, h, w, dtype, dev)
        L.check(lib.unet_bn_relu_apply(_DT[dtype], _ptr(y), pixels, co, _ptr(coef[2]), _ptr(coef[3]), _ptr(a), st),
                "unet_bn_relu_apply")
        ctx.save_for_backward(x, y, weight, gamma, coef)
        ctx.training = training
        ctx.out_sink = None
        ctx.out_link = None
        if out_link is not None and training:
            out_link.y, out_link.coef, out_link.dz_ptr = y, coef, 0
            ctx.out_link = out_link
        return a

    @staticmethod
    def backward(ctx, da):
        x, y, weight, gamma, coef = ctx.saved_tensors
        dtype = torch.bfloat16
        dt = _DT[dtype]
        n, ci, h, w = x.shape
        co, co_p = y.shape[1], weight.shape[0]
        narrow = co != co_p
        gkey, bkey = (0, 0) if narrow else (ctx.keys[2], ctx.keys[1])
        lib, st, dev = L.lib(), _stream(), x.device
        link = ctx.out_link
        dw, dgb = None, None
        if FUSE_FIRST_BN_BWD and link is not None and link.dz_ptr and link.dz_ptr == da.data_ptr() and da.dtype == dtype \
                and _is_nhwc(da) and ctx.training and ctx.needs_input_grad[1]:
            # The image layer's dy has ONE consumer, its weight gradient (nothing flows back into the image): the
            # BatchNorm-backward apply pass is folded into that kernel's operand -- finalize only (dy = NULL), then
            # unet_conv3x3_first_wgrad_bn streams dz and y and forms dy = A*dz + B*y + K per lane (bit-identical dW).
            dgb = (grad_out(gamma.shape, dev, gkey), grad_out(gamma.shape, dev, bkey))
            cf = torch.empty(3 * co, dtype=torch.float32, device=dev)
            L.check(lib.unet_bn_bwd_premasked(dt, None, None, n * h * w, co, _ptr(gamma), _ptr(coef[0]), _ptr(coef[1]),
                                              _ptr(link.partial), link.n_parts, _ptr(dgb[0]), _ptr(dgb[1]), None, _ptr(cf),
                                              cf.numel() * 4, st), "unet_bn_bwd_premasked(coefficients)")
            link.y = link.coef = link.partial = None
            link.dz_ptr = 0
            dw = torch.empty((co, ci, 3, 3), dtype=torch.float32, device=dev) if narrow else \
                grad_out(weight.shape, dev, ctx.keys[0])
            ws2 = _workspace(lib.unet_conv3x3_first_wgrad_workspace(n, h, w), dev)
            L.check(lib.unet_conv3x3_first_wgrad_bn(n, h, w, _ptr(x), ci, _ptr(da), _ptr(y), _ptr(cf), _ptr(dw), _ptr(ws2),
                                                    ws2.numel(), st), "unet_conv3x3_first_wgrad_bn")
        else:
            dy, dgb = _bn_relu_backward(lib, dt, dtype, da, y, gamma, coef, ctx.out_link, ctx.out_sink, dev, st,
                                        frozen=not ctx.training, beta_key=bkey, gamma_key=gkey)
            if ctx.needs_input_grad[1]:
                dw = torch.empty((co, ci, 3, 3), dtype=torch.float32, device=dev) if narrow else \
                    grad_out(weight.shape, dev, ctx.keys[0])
                need = lib.unet_conv3x3_first_wgrad_workspace(n, h, w)
                ws2 = _workspace(need, dev)
                L.check(lib.unet_conv3x3_first_wgrad(n, h, w, _ptr(x), ci, _ptr(dy), _ptr(dw), _ptr(ws2), ws2.numel(), st),
                        "unet_conv3x3_first_wgrad")
        if narrow:
            # padded gradients -> the parameters' shapes, one launch
            dgb_pad, dgb = dgb, (grad_out((co_p,), dev, ctx.keys[2]), grad_out((co_p,), dev, ctx.keys[1]))
            items = [_vec_item(L.REMAP_UNPAD, dgb_pad[0], dgb[0], co_p, co),
                     _vec_item(L.REMAP_UNPAD, dgb_pad[1], dgb[1], co_p, co)]
            if dw is not None:
                dw, dw_pad = grad_out(weight.shape, dev, ctx.keys[0]), dw
                items.append((L.REMAP_UNPAD, dw_pad, dw, co_p, ci, 9, co, ci, 0))
            _remap(items)
        return None, dw, dgb[0], dgb[1], None, None, None, None, None


FIRST_LAYER_KERNELS = __import__("os").environ.get("UNET_FIRST_LAYER", "1") != "0"
FUSE_FIRST_BN_BWD = __import__("os").environ.get("UNET_FUSE_FIRST_BN", "1") != "0"      # tuning hook (A/B runs)


def first_layer_ok(x: torch.Tensor, conv, dtype) -> bool:
    """The image layer qualifies for the one-MFMA-step kernels: bf16 mode, a plain fp32 NCHW image that needs no
    gradient, <= 3 channels into 64, width a multiple of 16."""
    return (FIRST_LAYER_KERNELS and dtype == torch.bfloat16 and x.dim() == 4 and x.dtype == torch.float32
            and not x.requires_grad and x.shape[1] == conv.in_channels
            and bool(L.lib().unet_conv3x3_first_supported(conv.in_channels, _pad64(conv.out_channels), x.shape[2],
                                                          x.shape[3])))


class ChannelDropout(torch.autograd.Function):
    """nn.Dropout2d on an NHWC activation (SegmentationUNet's bottleneck, /root/reference/src/model.py:129,146):
    ``noise`` = bernoulli(1-p)/(1-p) per (image, channel), drawn by the caller exactly as torch's feature dropout
    draws it; y = x * noise, dx = dy * noise (unet_channel_scale)."""

    @staticmethod
    def forward(ctx, x, noise):
        _require_cuda(x, noise)
        n, c, h, w = x.shape
        y = _nhwc_empty(n, c, h, w, x.dtype, x.device)
        L.check(L.lib().unet_channel_scale(_DT[x.dtype], _ptr(x), _ptr(noise), n, h * w, c, _ptr(y), _stream()),
                "unet_channel_scale")
        ctx.save_for_backward(noise)
        return y

    @staticmethod
    def backward(ctx, dy):
        (noise,) = ctx.saved_tensors
        n, c, h, w = dy.shape
        dy = _as_nhwc(dy, dy.dtype)
        dx = _nhwc_empty(n, c, h, w, dy.dtype, dy.device)
        L.check(L.lib().unet_channel_scale(_DT[dy.dtype], _ptr(dy), _ptr(noise), n, h * w, c, _ptr(dx), _stream()),
                "unet_channel_scale")
        return dx, None


def anomaly_score(reconstruction, original, l1=False):
    """(score map [N, H, W], image score [N]) of compute_anomaly_score (/root/reference/src/utils.py:205-215)."""
    _require_cuda(reconstruction, original)
    r = reconstruction.detach().contiguous().float()
    o = original.detach().contiguous().float()
    n, c = r.shape[0], r.shape[1]
    hw = int(r.numel() // (n * c))
    score = torch.empty((n,) + tuple(r.shape[2:]), dtype=torch.float32, device=r.device)
    img = torch.empty(n, dtype=torch.float32, device=r.device)
    lib = L.lib()
    ws = _workspace(lib.unet_anomaly_score_workspace(n, hw), r.device)
    L.check(lib.unet_anomaly_score(_ptr(r), _ptr(o), n, c, hw, 1 if l1 else 0, _ptr(score), _ptr(img), _ptr(ws), ws.numel(),
                                   _stream()), "unet_anomaly_score")
    return score, img


# ----------------------------------------------------------------------------- max pool
class MaxPool2(torch.autograd.Function):
    """nn.MaxPool2d(2) (/root/reference/src/model.py:32)."""

    @staticmethod
    def forward(ctx, x):
        _require_cuda(x)
        n, c, h, w = x.shape
        if h < 2 or w < 2:
            raise ValueError("MaxPool2d(2) needs at least 2x2 pixels")
        y = _nhwc_empty(n, c, h // 2, w // 2, x.dtype, x.device)
        L.check(L.lib().unet_maxpool2_fwd(_DT[x.dtype], _ptr(x), n, h, w, c, _ptr(y), _stream()), "unet_maxpool2_fwd")
        ctx.save_for_backward(x)
        ctx.sink = getattr(x, "_unet_sink", None)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        n, c, h, w = x.shape
        dy = _as_nhwc(dy, x.dtype)
        sink = ctx.sink
        fan_in = sink is not None and sink.begin(x.device)
        dx = sink.buf if fan_in else _nhwc_empty(n, c, h, w, x.dtype, x.device)
        L.check(L.lib().unet_maxpool2_bwd(_DT[x.dtype], _ptr(x), _ptr(dy), n, h, w, c, _ptr(dx), 1 if fan_in else 0,
                                          _stream()), "unet_maxpool2_bwd")
        if sink is not None:
            sink.done(dx, x.device)
            if fan_in:
                return None
        return dx


# ----------------------------------------------------------------------------- up-sampling
class ConvT2x2(torch.autograd.Function):
    """nn.ConvTranspose2d(Cin, Cin//2, kernel_size=2, stride=2) (/root/reference/src/model.py:51)."""

    @staticmethod
    def forward(ctx, x, weight, bias, in_link=None):
        """``in_link`` (BnLink, optional): ``x`` is the activation of a conv-BN-ReLU layer with no other consumer (the
        DoubleConv of the previous Up block): the data-gradient kernel then applies that layer's ReLU mask and reduces
        its BatchNorm-backward sums (unet_convt2x2_dgrad_bnrelu)."""
        _require_cuda(x, weight)
        n, ci, h, w = x.shape
        co = _pad64(weight.shape[1])          # narrow layer: zero weight rows / bias lanes
        dtype = x.dtype
        wp = packed(weight, L.PACK_CONVT_FWD, co, ci, dtype)
        if co != weight.shape[1]:
            bias_p = torch.empty(co, dtype=torch.float32, device=x.device)
            _remap([_vec_item(L.REMAP_PAD, bias.detach(), bias_p, weight.shape[1], co)])
            bias = bias_p
        y = _nhwc_empty(n, co, 2 * h, 2 * w, dtype, x.device)
        L.check(L.lib().unet_convt2x2_fwd(_DT[dtype], n, h, w, _ptr(x), ci, _ptr(wp), _ptr(bias), _ptr(y), co,
                                          _stream()), "unet_convt2x2_fwd")
        ctx.save_for_backward(x, weight)
        ctx.keys = (weight.data_ptr(), bias.data_ptr() if co == weight.shape[1] else 0)
        ctx.in_link = in_link if (in_link is not None and in_link.y is not None and
                                  in_link.y.data_ptr() != 0 and tuple(in_link.y.shape) == tuple(x.shape)) else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        n, ci, h, w = x.shape
        ci_p, co_p = weight.shape[0], weight.shape[1]
        co = _pad64(co_p)
        padded = (ci, co) != (ci_p, co_p)
        dtype = x.dtype
        lib, st, dev = L.lib(), _stream(), x.device
        dy = _as_nhwc(dy, dtype)
        dx = None
        if ctx.needs_input_grad[0]:
            wp = packed(weight, L.PACK_CONVT_DGRAD, ci, co, dtype)
            dx = _nhwc_empty(n, ci, h, w, dtype, dev)
            ilink = ctx.in_link if (FUSE_BN_BWD and FUSE_BN_CONVT) else None
            if ilink is not None and ilink.y is not None and \
                    lib.unet_convt2x2_dgrad_bnrelu_supported(_DT[dtype], n, h, w, ci, co):
                part = torch.empty((lib.unet_convt2x2_dgrad_bnrelu_max_parts(), 2, ci), dtype=torch.float32, device=dev)
                nparts = C.c_int32(0)
                pc = ilink.coef
                L.check(lib.unet_convt2x2_dgrad_bnrelu(_DT[dtype], n, h, w, _ptr(dy), co, _ptr(wp), _ptr(ilink.y),
                                                       _ptr(pc[2]), _ptr(pc[3]), _ptr(pc[0]), _ptr(dx), ci, _ptr(part),
                                                       C.byref(nparts), st), "unet_convt2x2_dgrad_bnrelu")
                ilink.partial, ilink.n_parts, ilink.dz_ptr = part, nparts.value, dx.data_ptr()
            else:
                L.check(lib.unet_convt2x2_dgrad(_DT[dtype], n, h, w, _ptr(dy), co, _ptr(wp), _ptr(dx), ci, st),
                        "unet_convt2x2_dgrad")
        if padded:
            dw = torch.empty((ci, co, 2, 2), dtype=torch.float32, device=dev)
            db = torch.empty(co, dtype=torch.float32, device=dev)
        else:
            dw = grad_out(weight.shape, dev, ctx.keys[0])
            db = grad_out((co,), dev, ctx.keys[1])
        ws = _workspace(lib.unet_convt2x2_wgrad_workspace(n, h, w, ci, co), dev)
        L.check(lib.unet_convt2x2_wgrad(_DT[dtype], n, h, w, _ptr(x), ci, _ptr(dy), co, _ptr(dw), _ptr(db),
                                        _ptr(ws), ws.numel(), st), "unet_convt2x2_wgrad")
        if padded:
            (dw, dw_pad), (db, db_pad) = (grad_out(weight.shape, dev, ctx.keys[0]), dw), (grad_out((co_p,), dev, 0), db)
            _remap([(L.REMAP_UNPAD, dw_pad, dw, ci_p, co_p, 4, ci, co, 0),
                    _vec_item(L.REMAP_UNPAD, db_pad, db, co_p, co)])
        return dx, dw, db, None


class Bilinear2x(torch.autograd.Function):
    """nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True) (/root/reference/src/model.py:48)."""

    @staticmethod
    def forward(ctx, x):
        _require_cuda(x)
        n, c, h, w = x.shape
        y = _nhwc_empty(n, c, 2 * h, 2 * w, x.dtype, x.device)
        L.check(L.lib().unet_upsample_bilinear2x_fwd(_DT[x.dtype], _ptr(x), n, h, w, c, _ptr(y), _stream()),
                "unet_upsample_bilinear2x_fwd")
        ctx.shape = (n, c, h, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        n, c, h, w = ctx.shape
        dy = _as_nhwc(dy, dy.dtype)
        dx = _nhwc_empty(n, c, h, w, dy.dtype, dy.device)
        L.check(L.lib().unet_upsample_bilinear2x_bwd(_DT[dy.dtype], _ptr(dy), n, h, w, c, _ptr(dx), _stream()),
                "unet_upsample_bilinear2x_bwd")
        return dx


# ----------------------------------------------------------------------------- 1x1 head
class Head(torch.autograd.Function):
    """OutConv (1x1 conv + bias, /root/reference/src/model.py:72) with the optional sigmoid of
    AnomalyUNet.forward (src/model.py:201,208).  Output: NCHW fp32."""

    @staticmethod
    def forward(ctx, x, weight, bias, sigmoid):
        _require_cuda(x, weight)
        n, ci, h, w = x.shape
        co = weight.shape[0]
        ctx.ci_p = weight.shape[1]
        if ci != ctx.ci_p:                    # padded input (a narrow OutConv): zero weight columns
            w_p = torch.empty((co, ci, 1, 1), dtype=torch.float32, device=x.device)
            _remap([(L.REMAP_PAD, weight.detach(), w_p, co, ctx.ci_p, 1, co, ci, 0)])
            weight = w_p
        out = torch.empty((n, co, h, w), dtype=torch.float32, device=x.device)
        L.check(L.lib().unet_head_fwd(_DT[x.dtype], _ptr(x), n, h, w, ci, _ptr(weight), _ptr(bias), co,
                                      int(sigmoid), _ptr(out), _stream()), "unet_head_fwd")
        ctx.save_for_backward(x, weight, out)
        ctx.sigmoid = bool(sigmoid)
        ctx.keys = (weight.data_ptr(), bias.data_ptr())
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, out = ctx.saved_tensors
        n, ci, h, w = x.shape
        co = weight.shape[0]
        lib, dev = L.lib(), x.device
        dout = dout.contiguous().float()
        dx = _nhwc_empty(n, ci, h, w, x.dtype, dev)
        padded = ci != ctx.ci_p
        dw = torch.empty((co, ci, 1, 1), dtype=torch.float32, device=dev) if padded else \
            grad_out(weight.shape, dev, ctx.keys[0])
        db = grad_out((co,), dev, ctx.keys[1])
        ws = _workspace(lib.unet_head_bwd_workspace(n, h, w, ci, co), dev)
        L.check(lib.unet_head_bwd(_DT[x.dtype], _ptr(x), _ptr(out), _ptr(dout), n, h, w, ci, _ptr(weight), co,
                                  int(ctx.sigmoid), _ptr(dx), _ptr(dw), _ptr(db), _ptr(ws), ws.numel(), _stream()),
                "unet_head_bwd")
        if padded:
            dw, dw_pad = grad_out((co, ctx.ci_p, 1, 1), dev, ctx.keys[0]), dw
            _remap([(L.REMAP_UNPAD, dw_pad, dw, co, ctx.ci_p, 1, co, ci, 0)])
        return dx, dw, db, None


# ----------------------------------------------------------------------------- losses
class MseFocal(torch.autograd.Function):
    """(MSE(recon, image), focal(amap, mask)) -- /root/reference/src/train_utils.py:23-35."""

    @staticmethod
    def forward(ctx, recon, amap, image, mask, alpha, gamma):
        _require_cuda(recon, amap, image, mask)
        recon, amap = recon.contiguous().float(), amap.contiguous().float()
        image, mask = image.contiguous().float(), mask.contiguous().float()
        if recon.shape != image.shape or amap.shape != mask.shape:
            raise ValueError("CombinedLoss: prediction/target shapes differ")
        lib, dev = L.lib(), recon.device
        losses = torch.empty(2, dtype=torch.float32, device=dev)
        d_recon, d_amap = torch.empty_like(recon), torch.empty_like(amap)
        ws = _workspace(lib.unet_loss_workspace(recon.numel()), dev)
        L.check(lib.unet_loss_mse_focal(_ptr(recon), _ptr(image), recon.numel(), _ptr(amap), _ptr(mask),
                                        amap.numel(), float(alpha), float(gamma), _ptr(losses), _ptr(d_recon),
                                        _ptr(d_amap), _ptr(ws), ws.numel(), _stream()), "unet_loss_mse_focal")
        ctx.save_for_backward(d_recon, d_amap)
        return losses[0], losses[1]

    @staticmethod
    def backward(ctx, g_mse, g_focal):
        d_recon, d_amap = ctx.saved_tensors
        return d_recon * g_mse, d_amap * g_focal, None, None, None, None


class Ssim(torch.autograd.Function):
    """SSIMLoss.forward (/root/reference/src/train_utils.py:89-104): a 0-d loss (size_average=True) or one value per
    image (size_average=False, :84-87)."""

    @staticmethod
    def forward(ctx, img1, img2, window_size, size_average=True):
        _require_cuda(img1, img2)
        img1, img2 = img1.contiguous().float(), img2.contiguous().float()
        n, c, h, w = img1.shape
        lib, dev = L.lib(), img1.device
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        d1 = torch.empty_like(img1) if need else None
        d2 = torch.empty_like(img2) if need else None
        ctx.per_image = not size_average
        if size_average:
            loss = torch.empty(1, dtype=torch.float32, device=dev)
            ws = _workspace(lib.unet_ssim_workspace(n * c, h, w), dev)
            L.check(lib.unet_ssim_loss(_ptr(img1), _ptr(img2), n * c, h, w, int(window_size), _ptr(loss), _ptr(d1),
                                       _ptr(d2), _ptr(ws), ws.numel(), _stream()), "unet_ssim_loss")
        else:
            loss = torch.empty(n, dtype=torch.float32, device=dev)
            ws = _workspace(lib.unet_ssim_workspace(c, h, w), dev)
            L.check(lib.unet_ssim_loss_per_image(_ptr(img1), _ptr(img2), n, c, h, w, int(window_size), _ptr(loss),
                                                 _ptr(d1), _ptr(d2), _ptr(ws), ws.numel(), _stream()),
                    "unet_ssim_loss_per_image")
        if need:
            ctx.save_for_backward(d1, d2)
        return loss[0] if size_average else loss

    @staticmethod
    def backward(ctx, g):
        d1, d2 = ctx.saved_tensors
        if ctx.per_image:
            g = g.reshape(-1, 1, 1, 1)
        return d1 * g, d2 * g, None, None


def threshold_confusion(pred, truth, thresholds, select=None, counts=None):
    """Confusion counts [K][4] = {tp, fp, fn, tn} (int64 DEVICE tensor; pass it back as ``counts`` to keep accumulating
    over batches, read it once at the end) of (pred > t) against (truth > 0.5) for each threshold, over the images with
    select[n] true (None: all): the pixel-metric epilogue of /root/reference/src/test.py:79-106 and
    src/train_utils.py:232-245 on the device (unet_threshold_confusion)."""
    _require_cuda(pred)
    p = pred.detach().contiguous().float()
    t = truth.detach().to(p.device).contiguous().float()
    if p.shape != t.shape or p.dim() < 2:
        raise ValueError("threshold_confusion: prediction / truth shapes differ")
    n = p.shape[0]
    per = p.numel() // n
    values = [float(v) for v in thresholds]
    if not values:
        raise ValueError("threshold_confusion: at least one threshold")
    sel = None if select is None else torch.as_tensor(select).to(device=p.device, dtype=torch.uint8).contiguous()
    if counts is None:
        counts = torch.zeros((len(values), 4), dtype=torch.int64, device=p.device)
    if tuple(counts.shape) != (len(values), 4):
        raise ValueError("threshold_confusion: counts must be [len(thresholds), 4]")
    for k in range(0, len(values), 8):           # the kernel takes up to 8 thresholds per pass over the maps
        thr = torch.tensor(values[k:k + 8], dtype=torch.float32, device=p.device)
        L.check(L.lib().unet_threshold_confusion(_ptr(p), _ptr(t), _ptr(sel), n, per, _ptr(thr), thr.numel(),
                                                 _ptr(counts[k:k + 8]), _stream()), "unet_threshold_confusion")
    return counts


def _select_runs(select, n, what):
    """(runs, device mask) of a per-image selection: a device mask goes to the kernels as it is (one run, all images); a
    host mask becomes one launch per run of selected images, so nothing is copied and nothing synchronises."""
    if select is None:
        return [(0, n)], None
    sel = torch.as_tensor(select)
    if sel.numel() != n:
        raise ValueError(f"{what}: select needs one entry per image")
    if sel.is_cuda:
        return [(0, n)], sel.reshape(-1).to(torch.uint8).contiguous()
    on = sel.reshape(-1).to(torch.bool).tolist() + [False]
    runs, start = [], None
    for i, v in enumerate(on):
        if v and start is None:
            start = i
        elif not v and start is not None:
            runs.append((start, i))
            start = None
    return runs, None


class BinaryAUC:
    """Pixel-level AUROC / AUPRC accumulated over batches: the roc_auc_score and auc(precision_recall_curve) that
    the reference src/utils.py:84-91 computes for calculate_pixel_metrics (:97-108), on the device.  A pixel is
    positive iff truth > 0.5; ties are float equality (-0.0 == +0.0).  ``update`` appends the selected pixels' scores
    as sort keys (unet_rank_auc_append) without synchronising; ``compute`` reads the counts once, sorts and ranks
    (unet_rank_auc).  No positives, no negatives or any NaN / inf score give 0.0 / 0.0, as calculate_metrics does when
    sklearn refuses.  The result depends only on the multiset of (score, label) pixels, bitwise."""

    def __init__(self):
        self._chunks = []                     # (keys, capacity, counts): one exactly-sized key chunk per update

    def update(self, pred, truth, select=None):
        """pred / truth: device tensors of equal shape [N, ...]; select: host or device bool per image (None: all)."""
        _require_cuda(pred)
        p = pred.detach().contiguous().float()
        t = truth.detach().to(p.device).contiguous().float()
        if p.shape != t.shape or p.dim() < 2:
            raise ValueError("BinaryAUC.update: prediction / truth shapes differ")
        n = p.shape[0]
        per = p.numel() // n
        runs, sel = _select_runs(select, n, "BinaryAUC.update")
        cap = sum(b - a for a, b in runs) * per
        if cap == 0:
            return
        keys = torch.empty(cap, dtype=torch.int32, device=p.device)
        counts = torch.zeros(3, dtype=torch.int64, device=p.device)
        lib = L.lib()
        for a, b in runs:
            L.check(lib.unet_rank_auc_append(_ptr(p[a:b]), _ptr(t[a:b]), _ptr(sel), b - a, per, _ptr(keys), cap,
                                             _ptr(counts), _stream()), "unet_rank_auc_append")
        self._chunks.append((keys, cap, counts))

    def compute(self):
        """{"auroc", "auprc", "positives", "negatives", "nonfinite"} over every pixel passed to update."""
        totals = [0, 0, 0]
        if self._chunks:
            per_chunk = torch.stack([c for _, _, c in self._chunks]).tolist()      # the one read of the counts
            totals = [sum(c[i] for c in per_chunk) for i in range(3)]
        n_pos, n_neg, nonfinite = totals
        res = {"auroc": 0.0, "auprc": 0.0, "positives": n_pos, "negatives": n_neg, "nonfinite": nonfinite}
        if nonfinite or not n_pos or not n_neg:
            return res
        lib = L.lib()
        nbytes = lib.unet_rank_auc_workspace(n_pos, n_neg)
        if nbytes == 0:
            raise RuntimeError(f"BinaryAUC: {n_pos + n_neg} pixels, at most 2^31 - 1 are supported")
        dev = self._chunks[0][0].device
        pos = torch.cat([k[:c[0]] for (k, _, _), c in zip(self._chunks, per_chunk)])          # copies: the sort
        neg = torch.cat([k[cap - c[1]:] for (k, cap, _), c in zip(self._chunks, per_chunk)])  # is in place
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty(2, dtype=torch.float64, device=dev)
        L.check(lib.unet_rank_auc(_ptr(pos), n_pos, _ptr(neg), n_neg, _ptr(out), _ptr(ws), nbytes, _stream()),
                "unet_rank_auc")
        res["auroc"], res["auprc"] = out.tolist()
        return res


def _image_planes(t, what):
    """[N, H, W] view of a [N, ..., H, W] tensor with one plane per image ([N, W]: one row)."""
    if t.dim() < 2:
        raise ValueError(f"{what}: needs [N, ...] maps")
    n, w = t.shape[0], t.shape[-1]
    h = t.shape[-2] if t.dim() >= 3 else 1
    if n == 0 or t.numel() != n * h * w:
        raise ValueError(f"{what}: one H x W plane per image, got {tuple(t.shape)}")
    return t.reshape(n, h, w)


def label_regions(truth, select=None, _runs=None):
    """8-connected regions of the defective pixels (truth > 0.5) of each image of truth [N, (1,) H, W], over the images
    with select[n] true (None: all): (labels, sizes, counts), all DEVICE tensors.  labels (int32, truth's shape) = 1 +
    the smallest linear index y * W + x of the pixel's region, sizes (int32) = the region's pixel count at each of its
    pixels, both 0 elsewhere; counts (int64 [3]) = {regions, defective pixels, ok pixels} of the selected images.
    scipy.ndimage.label(mask, np.ones((3, 3))) on the device (unet_label_regions); does not synchronise."""
    _require_cuda(truth)
    t = _image_planes(truth.detach().contiguous().float(), "label_regions")
    n, h, w = t.shape
    runs, sel = _runs if _runs is not None else _select_runs(select, n, "label_regions")
    lib = L.lib()
    labels = torch.zeros((n, h, w), dtype=torch.int32, device=t.device)
    sizes = torch.zeros((n, h, w), dtype=torch.int32, device=t.device)
    counts = torch.zeros(3, dtype=torch.int64, device=t.device)
    for a, b in runs:
        nbytes = lib.unet_label_regions_workspace(b - a, h, w)
        if nbytes == 0:
            raise RuntimeError(f"label_regions: {b - a} x {h} x {w} is not supported (n < 65536, at most 2^31 - 1 pixels)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=t.device)
        L.check(lib.unet_label_regions(_ptr(t[a:b]), _ptr(sel), b - a, h, w, _ptr(labels[a:b]), _ptr(sizes[a:b]),
                                       _ptr(counts), _ptr(ws), nbytes, _stream()), "unet_label_regions")
    return labels.reshape(truth.shape), sizes.reshape(truth.shape), counts


class RegionOverlapAUC:
    """AUPRO accumulated over batches: the area below the per-region-overlap curve of the MVTec AD evaluation up to a
    false-positive rate of ``fpr_limit``, divided by it.  A pixel is defective iff truth > 0.5, a region is an
    8-connected component of defective pixels of one image, and every region weighs the same: a defective pixel lifts
    the curve by 1 / (regions * its region's size).  ``update`` labels the batch's regions (unet_label_regions) and
    appends the selected pixels as sort keys and (key, size) elements (unet_region_auc_append) without synchronising;
    only those and the counts are kept.  ``compute`` reads the counts once, sorts and integrates (unet_region_auc).
    No region, no ok pixel or any NaN / inf score give 0.0.  The result depends only on the multiset of (score, region
    size) pixels, bitwise."""

    def __init__(self, fpr_limit=0.3):
        self.fpr_limit = float(fpr_limit)
        if not 0.0 < self.fpr_limit <= 1.0:
            raise ValueError(f"RegionOverlapAUC: fpr_limit {fpr_limit} is not in (0, 1]")
        self._chunks = []                     # (slots, capacity, counts[6]): one exactly-sized chunk per update
        self._max_region = 1

    def update(self, pred, truth, select=None):
        """pred / truth: device tensors of equal shape [N, (1,) H, W]; select: host or device bool per image."""
        _require_cuda(pred)
        p = pred.detach().contiguous().float()
        t = truth.detach().to(p.device).contiguous().float()
        if p.shape != t.shape:
            raise ValueError("RegionOverlapAUC.update: prediction / truth shapes differ")
        p = _image_planes(p, "RegionOverlapAUC.update")
        n, per = p.shape[0], p.shape[1] * p.shape[2]
        runs, sel = _select_runs(select, n, "RegionOverlapAUC.update")
        cap = sum(b - a for a, b in runs) * per
        if cap == 0:
            return
        _, sizes, regions = label_regions(t, _runs=(runs, sel))
        sizes = sizes.reshape(p.shape)
        slots = torch.empty(cap, dtype=torch.int64, device=p.device)
        counts = torch.zeros(3, dtype=torch.int64, device=p.device)
        lib = L.lib()
        for a, b in runs:
            L.check(lib.unet_region_auc_append(_ptr(p[a:b]), _ptr(sizes[a:b]), _ptr(sel), b - a, per, _ptr(slots), cap,
                                               _ptr(counts), _stream()), "unet_region_auc_append")
        self._chunks.append((slots, cap, torch.cat([counts, regions])))
        self._max_region = max(self._max_region, per)

    def compute(self):
        """{"aupro", "pro_at_limit", "fpr_limit", "regions", "defective", "ok", "nonfinite"} over every update."""
        totals = [0] * 6
        if self._chunks:
            per_chunk = torch.stack([c for _, _, c in self._chunks]).tolist()      # the one read of the counts
            totals = [sum(c[i] for c in per_chunk) for i in range(6)]
        n_pos, n_neg, nonfinite, regions, defective, ok = totals
        res = {"aupro": 0.0, "pro_at_limit": 0.0, "fpr_limit": self.fpr_limit, "regions": regions,
               "defective": defective, "ok": ok, "nonfinite": nonfinite}
        if nonfinite or not regions or not ok:
            return res
        lib = L.lib()
        nbytes = lib.unet_region_auc_workspace(n_pos, n_neg)
        if nbytes == 0:
            raise RuntimeError(f"RegionOverlapAUC: {n_pos + n_neg} pixels, at most 2^31 - 1 are supported")
        dev = self._chunks[0][0].device
        pos = torch.cat([s[:c[0]] for (s, _, _), c in zip(self._chunks, per_chunk)])          # copies: the sort
        neg = torch.cat([s.view(torch.int32)[2 * cap - c[1]:]                                 # destroys its input
                         for (s, cap, _), c in zip(self._chunks, per_chunk)])
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty(2, dtype=torch.float64, device=dev)
        L.check(lib.unet_region_auc(_ptr(pos), n_pos, _ptr(neg), n_neg, regions, self._max_region, self.fpr_limit,
                                    _ptr(out), _ptr(ws), nbytes, _stream()), "unet_region_auc")
        res["aupro"], res["pro_at_limit"] = out.tolist()
        return res


def _class_maps(labels, what):
    """uint8 [N, H, W] device maps of integer label maps; values outside 0..254 become 255 (background)."""
    _require_cuda(labels)
    t = labels.detach()
    if t.dtype != torch.uint8:
        if t.is_floating_point() or t.dtype == torch.bool:
            raise ValueError(f"{what}: integer label maps, got {t.dtype}")
        t = t.long()
        t = torch.where((t >= 0) & (t < 255), t, torch.full_like(t, 255)).to(torch.uint8)
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"{what}: [N, H, W] label maps, got {tuple(t.shape)}")
    return t.contiguous()


def _class_regions_error(what, n, h, w, num_classes):
    return RuntimeError(f"{what}: {n} x {h} x {w} maps of {num_classes} classes are not supported (n < 65536, at most "
                        "2^31 - 1 pixels, 2..255 classes)")


def label_class_regions(labels_u8, num_classes):
    """Class regions of integer label maps [N, H, W]: a pixel has class c iff its value is c with 1 <= c < num_classes
    (0 and every value >= num_classes, 255 among them, are background), and a class region is an 8-connected component
    of pixels of one class in one image.  Returns (region, sizes, counts), DEVICE tensors: region (int32 [N, H, W]) =
    1 + the smallest linear index y * W + x of the pixel's region, sizes (int32) = the region's pixel count at each of
    its pixels, both 0 on background; counts (int64 [N, num_classes]) = regions per image and class.  Per class,
    scipy.ndimage.label(map == c, np.ones((3, 3))) on the device (unet_label_class_regions); does not synchronise."""
    t = _class_maps(labels_u8, "label_class_regions")
    n, h, w = t.shape
    c = int(num_classes)
    lib = L.lib()
    nbytes = lib.unet_label_class_regions_workspace(n, h, w, c) if 0 <= c < 2 ** 31 else 0
    if nbytes == 0:
        raise _class_regions_error("label_class_regions", n, h, w, num_classes)
    region = torch.empty((n, h, w), dtype=torch.int32, device=t.device)
    sizes = torch.empty((n, h, w), dtype=torch.int32, device=t.device)
    counts = torch.zeros((n, c), dtype=torch.int64, device=t.device)
    ws = _workspace(nbytes, t.device)
    L.check(lib.unet_label_class_regions(_ptr(t), n, h, w, c, _ptr(region), _ptr(sizes), _ptr(counts), _ptr(ws),
                                         ws.numel(), _stream()), "unet_label_class_regions")
    return region, sizes, counts


RECORD_FIELDS = ("image", "class", "root", "size", "hit")


class ClassRegionMatcher:
    """Defect-level matching of predicted against true label maps, accumulated over batches.  Regions are those of
    ``label_class_regions``; a predicted region is kept iff it has at least ``min_pixels`` pixels.  ``hit`` of a truth
    region = its pixels whose predicted class is the region's and whose predicted region is kept; ``hit`` of a kept
    predicted region = its pixels whose truth class is its class (unet_match_class_regions; integers throughout).

    ``update`` labels truth and prediction in one call, matches them and keeps only the batch's two record buffers and
    its counts; it does not synchronise.  The buffers have to hold one record per pixel when they are made (the device
    alone knows how many regions there are), so the record counts travel to pinned host memory behind the kernels, and a
    later ``update`` trims every buffer whose counts have arrived, without waiting.  ``compute`` reads everything back
    once."""

    def __init__(self, num_classes, min_pixels=1):
        self.num_classes, self.min_pixels = int(num_classes), int(min_pixels)
        if not 2 <= self.num_classes <= 255:
            raise ValueError(f"ClassRegionMatcher: {num_classes} classes, 2..255 are supported")
        if self.min_pixels < 1:
            raise ValueError(f"ClassRegionMatcher: min_pixels {min_pixels} is below 1")
        self.images = 0
        self._chunks = []          # [truth records, pred records, class counts [2n, C], host counts, event or None]

    def _trim(self, wait):
        for ch in self._chunks:
            if ch[4] is None or not (wait or ch[4].query()):
                continue
            if wait:
                ch[4].synchronize()
            kt, kp = ch[3].tolist()
            if kt > ch[0].shape[0] or kp > ch[1].shape[0]:
                raise RuntimeError("ClassRegionMatcher: more records than pixels")      # cannot happen
            ch[0], ch[1], ch[4] = ch[0][:kt].clone(), ch[1][:kp].clone(), None

    def update(self, pred_labels, truth):
        """pred_labels / truth: integer device label maps of equal shape [N, H, W] (the uint8 argmax of
        ``metrics.per_image_stats(..., labels=True)`` and the loaders' masks; values outside 0..254 become 255)."""
        p = _class_maps(pred_labels, "ClassRegionMatcher.update")
        t = _class_maps(truth.to(p.device), "ClassRegionMatcher.update")
        if p.shape != t.shape:
            raise ValueError("ClassRegionMatcher.update: prediction / truth shapes differ")
        self._trim(wait=False)
        n, h, w = p.shape
        c, dev = self.num_classes, p.device
        region, sizes, class_counts = label_class_regions(torch.cat([t, p]), c)      # one pass labels both
        lib = L.lib()
        nbytes = lib.unet_match_class_regions_workspace(n, h, w, c)
        if nbytes == 0 or self.images + n >= 2 ** 31:
            raise _class_regions_error("ClassRegionMatcher.update", n, h, w, c)
        cap = n * h * w
        records = [torch.empty((cap, len(RECORD_FIELDS)), dtype=torch.int32, device=dev) for _ in range(2)]
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        ws = _workspace(nbytes, dev)
        L.check(lib.unet_match_class_regions(_ptr(t), _ptr(region[:n]), _ptr(sizes[:n]), _ptr(p), _ptr(region[n:]),
                                             _ptr(sizes[n:]), n, h, w, c, self.min_pixels, self.images,
                                             _ptr(records[0]), _ptr(records[1]), cap, _ptr(counts), _ptr(ws),
                                             ws.numel(), _stream()), "unet_match_class_regions")
        host = torch.empty(2, dtype=torch.int64, pin_memory=True)
        host.copy_(counts, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self._chunks.append([records[0], records[1], class_counts, host, done])
        self.images += n

    def compute(self):
        """{"truth", "pred"}: int32 [K, 5] numpy records (image, class, root index y * W + x, size, hit), the image index
        counted over all updates, sorted by (image, root index); {"truth_counts", "pred_counts"}: int64
        [images, num_classes] regions per image and class (pred_counts before the min_pixels rule); "images"."""
        import numpy as np
        c, f = self.num_classes, len(RECORD_FIELDS)
        empty = np.zeros((0, f), np.int32)
        res = {"truth": empty, "pred": empty.copy(), "truth_counts": np.zeros((0, c), np.int64),
               "pred_counts": np.zeros((0, c), np.int64), "images": self.images}
        if not self._chunks:
            return res
        self._trim(wait=True)
        parts = [ch[0].reshape(-1) for ch in self._chunks] + [ch[1].reshape(-1) for ch in self._chunks]
        parts += [ch[2].to(torch.int32).reshape(-1) for ch in self._chunks]          # a count is below 2^31 pixels
        flat = torch.cat(parts).cpu().numpy()                                       # the one read-back
        kt = sum(ch[0].shape[0] for ch in self._chunks) * f
        kp = sum(ch[1].shape[0] for ch in self._chunks) * f
        for key, rec in (("truth", flat[:kt]), ("pred", flat[kt:kt + kp])):
            rec = rec.reshape(-1, f)
            res[key] = np.ascontiguousarray(rec[np.lexsort((rec[:, 2], rec[:, 0]))])
        at, tc, pc = kt + kp, [], []
        for ch in self._chunks:
            n = ch[2].shape[0] // 2
            both = flat[at:at + 2 * n * c].reshape(2, n, c).astype(np.int64)
            tc.append(both[0]); pc.append(both[1])
            at += 2 * n * c
        res["truth_counts"], res["pred_counts"] = np.concatenate(tc), np.concatenate(pc)
        return res


def preprocess_u8(images_u8, flips=None, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """uint8 [N, H, W, 3] device batch -> normalised fp32 NCHW (ToTensor + Normalize, optional per-sample horizontal
    flip): /root/reference/src/dataset.py:134-146, src/kolektorsdd_dataset.py:133-150, on the GPU."""
    _require_cuda(images_u8)
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3:
        raise ValueError("preprocess_u8 expects a uint8 [N, H, W, 3] tensor")
    images_u8 = images_u8.contiguous()
    n, h, w, _ = images_u8.shape
    out = torch.empty((n, 3, h, w), dtype=torch.float32, device=images_u8.device)
    fl = None
    if flips is not None:
        fl = flips.to(device=images_u8.device, dtype=torch.uint8).contiguous()
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s_ = (C.c_float * 3)(*[float(v) for v in std])
    L.check(L.lib().unet_preprocess_u8(_ptr(images_u8), _ptr(fl), _ptr(out), n, h, w, m, s_, _stream()),
            "unet_preprocess_u8")
    return out


# ----------------------------------------------------------------------------- visualisation sheet
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # reference src/utils.py:21
_PANEL_KINDS = {"image": L.PANEL_IMAGE, "unit": L.PANEL_UNIT, "gray": L.PANEL_GRAY, "hot": L.PANEL_HOT,
                "overlay": L.PANEL_OVERLAY}
MAX_PANELS = 8
# matplotlib's `hot` (_cm.py _hot_data): per channel the (x, y) knots of a piecewise-linear map
_HOT_KNOTS = (((0.0, 0.0416), (0.365079, 1.0), (1.0, 1.0)),
              ((0.0, 0.0), (0.365079, 0.0), (0.746032, 1.0), (1.0, 1.0)),
              ((0.0, 0.0), (0.746032, 0.0), (1.0, 1.0)))
_luts = {}                 # device index -> uint8 [2][256][3] (gray, hot), uploaded once


def colormap_lut(name):
    """The 256 RGB byte triples of matplotlib's `gray` or `hot` as a list of tuples, in host float64 (Python floats):
    floor(255 * L(x_k)) at x_k = k * (1 / 255), x_255 = 1 -- the abscissae as numpy's linspace forms them, so 255 * x_k
    falls below k for some k and gray is not simply (k, k, k).  L is linear between the knots, in matplotlib's
    operation order.  matplotlib itself is not needed."""
    if name not in ("gray", "hot"):
        raise ValueError(f"colormap_lut: no table for {name!r}")

    def level(knots, x):
        for (x0, y0), (x1, y1) in zip(knots, knots[1:]):
            if x <= x1:
                return ((x - x0) / (x1 - x0)) * (y1 - y0) + y0
        return knots[-1][1]

    step = 1.0 / 255.0
    out = []
    for k in range(256):
        x = k * step if k < 255 else 1.0
        vals = (x, x, x) if name == "gray" else tuple(level(kn, x) for kn in _HOT_KNOTS)
        out.append(tuple(int(255.0 * min(max(v, 0.0), 1.0)) for v in vals))      # (int() floors: nothing is negative)
    return out


def _render_luts(device):
    key = device.index if device.index is not None else torch.cuda.current_device()
    t = _luts.get(key)
    if t is None:
        t = torch.tensor([colormap_lut("gray"), colormap_lut("hot")], dtype=torch.uint8).to(device)
        _luts[key] = t
    return t


def _map_planes(t, what):
    if not (t.dim() == 3 or (t.dim() == 4 and t.shape[1] == 1)):
        raise ValueError(f"{what}: a map is (N, 1, H, W) or (N, H, W), got {tuple(t.shape)}")
    return t.shape[0], t.shape[-2], t.shape[-1]


def _panels(columns, what):
    """Checks `columns` and returns (descriptors, n, h, w, tensors kept alive): nothing is launched before this passes."""
    columns = list(columns)
    if not 1 <= len(columns) <= MAX_PANELS:
        raise ValueError(f"{what}: 1 to {MAX_PANELS} columns, got {len(columns)}")
    parsed, shape, dev = [], None, None
    for col in columns:
        kind = col[0]
        if kind not in _PANEL_KINDS or len(col) != (4 if kind == "overlay" else 2):
            raise ValueError(f"{what}: a column is (kind, tensor) with kind in image / unit / gray / hot, or "
                             f"('overlay', image, map, alpha); got {col[0]!r} with {len(col) - 1} values")
        rgb = col[1] if kind in ("image", "unit", "overlay") else None
        amap = col[2] if kind == "overlay" else (col[1] if rgb is None else None)
        a8 = 0
        if kind == "overlay":
            if not 0.0 <= float(col[3]) <= 1.0:
                raise ValueError(f"{what}: overlay alpha {col[3]} is not in [0, 1]")
            a8 = int(round(255 * float(col[3])))
        _require_cuda(rgb, amap)
        for t, is_rgb in ((rgb, True), (amap, False)):
            if t is None:
                continue
            if is_rgb:
                if t.dim() != 4 or t.shape[1] != 3:
                    raise ValueError(f"{what}: an {kind} input is (N, 3, H, W), got {tuple(t.shape)}")
                nhw = (t.shape[0], t.shape[2], t.shape[3])
            else:
                nhw = _map_planes(t, what)
            if min(nhw) < 1:
                raise ValueError(f"{what}: empty input {tuple(t.shape)}")
            shape, dev = shape or nhw, dev or t.device
            if nhw != shape or t.device != dev:
                raise ValueError(f"{what}: all columns share N, H, W and the device; got {nhw} on {t.device} after "
                                 f"{shape} on {dev}")
        parsed.append((kind, rgb, amap, a8))
    descs, keep = (L.Panel * len(parsed))(), []
    for i, (kind, rgb, amap, a8) in enumerate(parsed):
        ptrs = []
        for t in (rgb, amap):
            if t is not None:
                t = t.detach().float().contiguous()          # bf16 outputs are upcast; fp32 contiguous ones pass as they are
                keep.append(t)
            ptrs.append(None if t is None else t.data_ptr())
        descs[i] = L.Panel(_PANEL_KINDS[kind], a8, ptrs[0], ptrs[1])
    return descs, shape, keep


def panel_range(t):
    """(N, 2) fp32 DEVICE tensor: the smallest and the largest finite value of each plane of t (N, 1, H, W) or (N, H, W),
    NaN / NaN for a plane without a finite pixel; -0.0 and +0.0 may fold.  The range pass of render_sheet on its own
    (unet_render_range: integer atomics on order-preserving keys); does not synchronise."""
    _require_cuda(t)
    descs, (n, h, w), keep = _panels([("gray", t)], "panel_range")
    keys = torch.empty((2, n), dtype=torch.int32, device=t.device)
    L.check(L.lib().unet_render_range(descs, 1, n, h, w, _ptr(keys), _stream()), "unet_render_range")
    k = keys.to(torch.int64) & 0xFFFFFFFF                    # the key transform, undone
    bits = torch.where(k >= 1 << 31, k - (1 << 31), 0xFFFFFFFF - k)
    vals = bits.to(torch.int32).view(torch.float32)
    vals = torch.where((k[0] > k[1]).unsqueeze(0), torch.full_like(vals, float("nan")), vals)
    return vals.t().contiguous()


def render_sheet(columns, gutter=4, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """The visualisation sheet of visualize_results (/root/reference/src/utils.py:111-157) as a uint8 DEVICE tensor
    (N H + (N - 1) gutter, K W + (K - 1) gutter, 3): one row per sample, one panel per column, `gutter` pixels of 255
    between panels.  columns: up to 8 of ("image", t) -- ImageNet-normalised (N, 3, H, W), denormalised with mean / std
    and clamped --, ("unit", t) -- (N, 3, H, W) clamped to [0, 1] --, ("gray", t) / ("hot", t) -- (N, 1, H, W) maps, each
    plane scaled to its own finite range and sent through matplotlib's table --, ("overlay", image, map, alpha) -- the
    hot map blended over the image, 0 <= alpha <= 1.  Bytes equal matplotlib's (see include/unet_hip.h).  Two launches
    (unet_render_range, unet_render_sheet); does not synchronise."""
    descs, (n, h, w), keep = _panels(columns, "render_sheet")
    gutter = int(gutter)
    if gutter < 0:
        raise ValueError(f"render_sheet: gutter {gutter} is negative")
    dev = keep[0].device
    k = len(descs)
    rows, cols = n * h + (n - 1) * gutter, k * w + (k - 1) * gutter
    if rows * cols * 3 >= 1 << 31:
        raise ValueError(f"render_sheet: a sheet of {rows} x {cols} pixels (fewer than 2^31 bytes are supported)")
    luts = _render_luts(dev)
    keys = torch.empty((2, k, n), dtype=torch.int32, device=dev)
    sheet = torch.empty((rows, cols, 3), dtype=torch.uint8, device=dev)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s_ = (C.c_float * 3)(*[float(v) for v in std])
    lib = L.lib()
    L.check(lib.unet_render_range(descs, k, n, h, w, _ptr(keys), _stream()), "unet_render_range")
    L.check(lib.unet_render_sheet(descs, k, n, h, w, gutter, m, s_, _ptr(keys), _ptr(luts), _ptr(sheet), _stream()),
            "unet_render_sheet")
    return sheet


# ----------------------------------------------------------------------------- segmentation prediction sheets
_SEG_PANEL_KINDS = {"image": L.SEG_PANEL_IMAGE, "classes": L.SEG_PANEL_CLASSES, "overlay": L.SEG_PANEL_OVERLAY,
                    "lut": L.SEG_PANEL_LUT}
# matplotlib's `tab10` (colormaps['tab10'](i, bytes=True), matplotlib 3.10.8)
TAB10 = ((31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189), (140, 86, 75), (227, 119, 194),
         (127, 127, 127), (188, 189, 34), (23, 190, 207))
_seg_tables = {}           # (device index, "palette" | "lut") -> the default table, uploaded once


def seg_confidence(logits, labels=True, conf=True):
    """(labels, conf) of (N, C, H, W) logits, 2 <= C <= 8, as DEVICE tensors: labels uint8 (N, H, W) = the argmax (the
    first maximum wins ties, as torch.argmax), conf float32 (N, H, W) = softmax(logits, 1).max(1) computed in fp32 as
    1 / sum_j expf(z_j - max z) (reference visualize.py:134-135, visualize_kolektorsdd.py:131).  Either is None
    when not asked for.  One launch (unet_seg_confidence); does not synchronise."""
    _require_cuda(logits)
    if logits.dim() != 4:
        raise ValueError(f"seg_confidence: logits are (N, C, H, W), got {tuple(logits.shape)}")
    if not (labels or conf):
        raise ValueError("seg_confidence: neither labels nor conf asked for")
    n, c, h, w = logits.shape
    x = logits.detach().float().contiguous()
    lab = torch.empty((n, h, w), dtype=torch.uint8, device=x.device) if labels else None
    cf = torch.empty((n, h, w), dtype=torch.float32, device=x.device) if conf else None
    L.check(L.lib().unet_seg_confidence(_ptr(x), n, c, h * w, _ptr(lab), _ptr(cf), _stream()), "unet_seg_confidence")
    return lab, cf


def class_palette(num_classes, mode):
    """(256, 3) uint8 host tensor: the colour of every label byte, `tab10` for classes 0 .. num_classes - 1 and white
    above.  mode "index": class i takes tab10 entry i (Gear: cmap(i), reference visualize.py:75-83); mode "scaled":
    entry min(floor(i / (C - 1) * 10), 9) (KolektorSDD: imshow(cmap='tab10', vmin=0, vmax=C - 1),
    visualize_kolektorsdd.py:118).  matplotlib is not needed."""
    c = int(num_classes)
    if not 2 <= c <= 10:
        raise ValueError(f"class_palette: 2 to 10 classes (tab10), got {num_classes}")
    if mode not in ("index", "scaled"):
        raise ValueError(f"class_palette: mode is 'index' or 'scaled', got {mode!r}")
    rows = [TAB10[i if mode == "index" else min(int(i / (c - 1) * 10), 9)] for i in range(c)]
    return torch.tensor(rows + [(255, 255, 255)] * (256 - c), dtype=torch.uint8)


def viridis_lut():
    """(256, 3) uint8 host tensor: matplotlib's `viridis` (a listed colour map: the bytes are embedded, _viridis.py,
    generated by tools/make_viridis_table.py)."""
    from ._viridis import VIRIDIS
    return torch.frombuffer(bytearray(VIRIDIS), dtype=torch.uint8).reshape(256, 3)


def _seg_table(t, default, dev, what):
    """A (256, 3) uint8 table on `dev`: the caller's, or the default (built and uploaded once per device)."""
    if t is None:
        key = (dev.index if dev.index is not None else torch.cuda.current_device(), what)
        t = _seg_tables.get(key)
        if t is None:
            t = _seg_tables[key] = default().to(dev)
        return t
    return t.to(device=dev).contiguous()


def _seg_panels(images, columns, gutter, per_row, palette, lut, what):
    """Checks every argument of render_seg_sheet and returns (parsed columns, n, h, w): nothing is launched, converted
    or looked up in the library before this passes.  Shapes and values first, the device last."""
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 3 or not images.is_floating_point():
        raise ValueError(f"{what}: images are a float (N, 3, H, W) tensor, got "
                         f"{tuple(images.shape) if torch.is_tensor(images) else type(images).__name__}")
    n, _, h, w = images.shape
    if min(n, h, w) < 1:
        raise ValueError(f"{what}: empty images {tuple(images.shape)}")
    columns = list(columns)
    if not 1 <= len(columns) <= MAX_PANELS:
        raise ValueError(f"{what}: 1 to {MAX_PANELS} columns, got {len(columns)}")
    if int(gutter) != gutter or gutter < 0:
        raise ValueError(f"{what}: gutter {gutter} is not a non-negative integer")
    if int(per_row) != per_row or per_row < 1:
        raise ValueError(f"{what}: per_row {per_row} is not a positive integer")
    arity = {"image": 1, "classes": 2, "overlay": 3, "lut": 2}
    parsed, tensors = [], [images]
    for col in columns:
        col = tuple(col)
        kind = col[0] if col else None
        if kind not in arity or len(col) != arity[kind]:
            raise ValueError(f"{what}: a column is ('image',), ('classes', labels), ('overlay', labels, alpha) or "
                             f"('lut', map); got {kind!r} with {max(len(col) - 1, 0)} values")
        t, a8 = (col[1] if len(col) > 1 else None), 0
        if kind in ("classes", "overlay"):
            if not torch.is_tensor(t) or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
                raise ValueError(f"{what}: {kind} labels are an integer tensor (uint8, or int64 masks)")
        elif kind == "lut":
            if not torch.is_tensor(t) or not t.is_floating_point():
                raise ValueError(f"{what}: a lut map is a float tensor")
        if t is not None:
            if tuple(t.shape) != (n, h, w):
                raise ValueError(f"{what}: a {kind} input is (N, H, W) = {(n, h, w)}, got {tuple(t.shape)}")
            tensors.append(t)
        if kind == "overlay":
            if not 0.0 <= float(col[2]) <= 1.0:
                raise ValueError(f"{what}: overlay alpha {col[2]} is not in [0, 1]")
            a8 = int(round(255 * float(col[2])))
        parsed.append((kind, t, a8))
    rows_, cells = -(-n // int(per_row)), int(per_row) * len(parsed)
    rows, cols = rows_ * h + (rows_ - 1) * int(gutter), cells * w + (cells - 1) * int(gutter)
    if n >= 65536 or rows * cols * 3 >= 1 << 31:
        raise ValueError(f"{what}: {n} samples on a sheet of {rows} x {cols} pixels (fewer than 65536 samples and 2^31 "
                         "bytes are supported)")
    for name, t in (("palette", palette), ("lut", lut)):
        if t is not None and not (torch.is_tensor(t) and t.dtype == torch.uint8 and tuple(t.shape) == (256, 3)):
            raise ValueError(f"{what}: {name} is a (256, 3) uint8 tensor")
    _require_cuda(*tensors)
    if any(t.device != images.device for t in tensors):
        raise ValueError(f"{what}: images and columns share one device")
    return parsed, n, h, w, rows, cols


def render_seg_sheet(images, columns, gutter=4, per_row=1, palette=None, lut=None):
    """The prediction sheet of the Gear / KolektorSDD visualisers (reference visualize.py:120-236,
    visualize_kolektorsdd.py:101-202) as a uint8 DEVICE tensor (rows, cols, 3): ceil(N / per_row) rows of per_row
    samples, each sample its columns side by side, `gutter` pixels of 255 between panels in both directions and in the
    cells past N.  images: ImageNet-normalised (N, 3, H, W).  columns: up to 8 of ("image",) -- denormalised and clamped
    --, ("classes", labels) -- palette[label] --, ("overlay", labels, alpha) -- the palette colour blended over the
    image where the label is not 0 (this package's integer blend, not Agg's compositing) --, ("lut", map) -- a float
    (N, H, W) map over the fixed range [0, 1] through `lut`, non-finite pixels white.  labels: uint8 (N, H, W); other
    integer dtypes (int64 masks) are converted, values outside 0..255 becoming 255, which the default palettes draw
    white.  palette / lut: (256, 3) uint8, default class_palette(10, "index") / viridis_lut().  One launch
    (unet_seg_render_sheet); does not synchronise."""
    what = "render_seg_sheet"
    parsed, n, h, w, rows, cols = _seg_panels(images, columns, gutter, per_row, palette, lut, what)
    dev = images.device
    x = images.detach().float().contiguous()
    descs, keep = (L.SegPanel * len(parsed))(), [x]
    for i, (kind, t, a8) in enumerate(parsed):
        lab = amap = None
        if kind in ("classes", "overlay"):
            lab = t.detach()
            if lab.dtype != torch.uint8:
                lab = torch.where((lab < 0) | (lab > 255), torch.full_like(lab, 255), lab).to(torch.uint8)
            lab = lab.contiguous()
            keep.append(lab)
        elif kind == "lut":
            amap = t.detach().float().contiguous()
            keep.append(amap)
        descs[i] = L.SegPanel(_SEG_PANEL_KINDS[kind], a8, None if lab is None else lab.data_ptr(),
                              None if amap is None else amap.data_ptr())
    pal = _seg_table(palette, lambda: class_palette(10, "index"), dev, "palette")
    table = _seg_table(lut, viridis_lut, dev, "lut")
    sheet = torch.empty((rows, cols, 3), dtype=torch.uint8, device=dev)
    m = (C.c_float * 3)(*[float(v) for v in IMAGENET_MEAN])
    s_ = (C.c_float * 3)(*[float(v) for v in IMAGENET_STD])
    L.check(L.lib().unet_seg_render_sheet(_ptr(x), descs, len(parsed), n, h, w, int(gutter), int(per_row), m, s_,
                                          _ptr(pal), _ptr(table), _ptr(sheet), _stream()), "unet_seg_render_sheet")
    return sheet


# ----------------------------------------------------------------------------- profiling / optimiser
def prof_enable(on: bool) -> None:
    L.check(L.lib().unet_prof_enable(int(on)), "unet_prof_enable")


def prof_collect():
    ms = (C.c_double * L.K_COUNT)()
    launches = (C.c_int64 * L.K_COUNT)()
    flops = (C.c_double * L.K_COUNT)()
    L.check(L.lib().unet_prof_collect(ms, launches, flops), "unet_prof_collect")
    return {L.KCLASS_NAMES[i]: {"ms": ms[i], "launches": launches[i], "flops": flops[i]}
            for i in range(L.K_COUNT)}


def prof_kernels():
    """Per-kernel breakdown of the brackets consumed by the last prof_collect(): {kernel name: ms, launches, flops}."""
    out, i = {}, 0
    lib = L.lib()
    while True:
        name, ms, n, fl = C.c_char_p(), C.c_double(), C.c_int64(), C.c_double()
        if lib.unet_prof_kernel_stats(i, C.byref(name), C.byref(ms), C.byref(n), C.byref(fl)) != 0:
            break
        by = C.c_double()
        lib.unet_prof_kernel_bytes(i, C.byref(by))
        out[name.value.decode()] = {"ms": ms.value, "launches": n.value, "flops": fl.value, "bytes": by.value}
        i += 1
    return out


def adam_step_(param, grad, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, weight_decay, grad_scale=1.0):
    """In-place fused Adam over flat fp32 arenas (torch.optim.Adam semantics, train_utils.py:266)."""
    _require_cuda(param, grad, exp_avg, exp_avg_sq)
    L.check(L.lib().unet_adam_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(),
                                   lr, beta1, beta2, eps, weight_decay, grad_scale, int(step), _stream()),
            "unet_adam_step")
    parameters_written()                   # raw-pointer update: no version counter moved
