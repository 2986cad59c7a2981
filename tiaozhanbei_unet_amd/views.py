"""Test-time view ensembling (no reference counterpart): the model runs on several views of an image -- the image resized
by a factor, possibly mirrored -- and the views' logits are brought back onto one frame and averaged on the device
(csrc/views.hip: unet_view_merge; restated by tests/_views_ref.py).

``plan_views`` lists the views (plain integers and floats: importable and testable without a GPU), ``merge_views`` is the
launch, ``ViewEnsemble`` strings both around a ``tiling.TiledPredictor``.
"""
from __future__ import annotations

import torch

from . import _lib as L
from ._hipcall import _ptr, _require_cuda, _stream

MAX_VIEWS = 16               # unet_view_merge: views per call
MAX_SIDE = 16384             # unet_view_merge: the longest side of the frame and of a view
MIN_SCALE, MAX_SCALE = 0.5, 2.0
FLIP_SETS = {"none": ((0, 0),), "h": ((0, 0), (1, 0)), "v": ((0, 0), (0, 1)), "all": ((0, 0), (1, 0), (0, 1), (1, 1))}


def plan_views(scales, flips):
    """The ordered views ``[(scale, flip_x, flip_y)]``: the scales in the order given, each in [0.5, 2], and per scale the
    flips of the set ``flips`` in the order none, x, y, xy -- ``none``, ``h`` (none + x), ``v`` (none + y) or ``all``.
    Duplicates are dropped; ValueError for an unknown set, no scale, a scale out of range or more than 16 views."""
    if flips not in FLIP_SETS:
        raise ValueError(f"plan_views: flips {flips!r} is not one of {sorted(FLIP_SETS)}")
    views = []
    for s in scales:
        s = float(s)
        if not MIN_SCALE <= s <= MAX_SCALE:
            raise ValueError(f"plan_views: scale {s} is not in [{MIN_SCALE}, {MAX_SCALE}]")
        for fx, fy in FLIP_SETS[flips]:
            if (s, fx, fy) not in views:
                views.append((s, fx, fy))
    if not views:
        raise ValueError("plan_views: no scale was given")
    if len(views) > MAX_VIEWS:
        raise ValueError(f"plan_views: {len(views)} views (at most {MAX_VIEWS})")
    return views


def merge_views(view_logits, flips, frame_hw, merged=False, labels=True, conf=True, agreement=True):
    """(labels, conf, agreement[, merged]) of a frame (H, W) from the float32 DEVICE logits (C, hv, wv) of 1 to 16 views,
    2 <= C <= 8, each of its own size (sides 1 to 16384), and ``flips``, per view (flip_x, flip_y): whether the model saw
    the image mirrored along x / y.  Every view is sampled at the frame's pixel centres (bilinear in 16.16 taps with edge
    clamp, a view of the frame's own size unchanged), mirrored back, and the logits are averaged: merged float32
    (C, H, W); labels uint8 (H, W) and conf float32 (H, W) follow by ``sheets.seg_confidence``'s rule; agreement uint8
    (H, W) counts the views whose own first maximum is the merged label.  An output that is switched off is None (not all
    of them may be).  One launch (unet_view_merge); does not synchronise."""
    what = "merge_views"
    view_logits, flips = list(view_logits), [tuple(int(bool(v)) for v in f) for f in flips]
    if not 1 <= len(view_logits) <= MAX_VIEWS:
        raise ValueError(f"{what}: {len(view_logits)} views (1 to {MAX_VIEWS})")
    if len(flips) != len(view_logits) or any(len(f) != 2 for f in flips):
        raise ValueError(f"{what}: {len(flips)} (flip_x, flip_y) pairs for {len(view_logits)} views")
    for z in view_logits:
        if not torch.is_tensor(z) or z.dim() != 3 or z.dtype != torch.float32:
            raise ValueError(f"{what}: a view's logits are a float32 (C, hv, wv) tensor, got "
                             f"{(tuple(z.shape), z.dtype) if torch.is_tensor(z) else type(z).__name__}")
    c = int(view_logits[0].shape[0])
    if any(int(z.shape[0]) != c for z in view_logits):
        raise ValueError(f"{what}: the views have {[int(z.shape[0]) for z in view_logits]} classes")
    if any(z.device != view_logits[0].device for z in view_logits):
        raise ValueError(f"{what}: the views share one device")
    h, w = (int(v) for v in frame_hw)
    if not (merged or labels or conf or agreement):
        raise ValueError(f"{what}: every output is switched off")
    _require_cuda(*view_logits)
    zs = [z.detach().contiguous() for z in view_logits]
    desc = (L.MergeView * len(zs))(*[L.MergeView(z.data_ptr(), z.shape[1], z.shape[2], fx, fy)
                                     for z, (fx, fy) in zip(zs, flips)])
    dev = zs[0].device
    out_labels = torch.empty((h, w), dtype=torch.uint8, device=dev) if labels else None
    out_conf = torch.empty((h, w), dtype=torch.float32, device=dev) if conf else None
    out_agree = torch.empty((h, w), dtype=torch.uint8, device=dev) if agreement else None
    out_merged = torch.empty((c, h, w), dtype=torch.float32, device=dev) if merged else None
    L.check(L.lib().unet_view_merge(desc, len(zs), c, h, w, _ptr(out_merged), _ptr(out_labels), _ptr(out_conf),
                                    _ptr(out_agree), _stream()), "unet_view_merge")
    return (out_labels, out_conf, out_agree, out_merged) if merged else (out_labels, out_conf, out_agree)


class ViewEnsemble:
    """``predictor`` (a ``tiling.TiledPredictor``) over the views ``[(scale, flip_x, flip_y)]`` of ``plan_views``:
    ``__call__(image_u8, frame_hw)`` takes a decoded uint8 DEVICE image (H0, W0, 3) and the output frame (H, W) and returns
    (labels uint8 (H, W), conf float32 (H, W), agreement uint8 (H, W), plan).  Per view the image is resized to
    ``predict_tiled.working_frame(frame_hw, scale)`` (``augment.resize_bilinear_u8``, skipped when it has that size already),
    normalised (``augment.color_jitter_normalize_u8``), mirrored (``torch.flip`` of the float frame) and run through
    ``predictor.blended_logits``; one launch merges the views' logits onto the frame.  plan: per view ``{"scale",
    "flip_x", "flip_y", "frame_size": [hv, wv], "tiling": the predictor's tile plan}``.  One image at a time."""

    def __init__(self, predictor, views):
        self.predictor = predictor
        self.views = [(float(s), int(bool(fx)), int(bool(fy))) for s, fx, fy in views]
        if not 1 <= len(self.views) <= MAX_VIEWS:
            raise ValueError(f"ViewEnsemble: {len(self.views)} views (1 to {MAX_VIEWS})")

    def view_logits(self, image_u8, frame_hw):
        """([logits float32 (C, hv, wv) per view], plan): what ``predictor.blended_logits`` makes of every view"""
        from . import augment
        from .predict_tiled import working_frame
        if not torch.is_tensor(image_u8) or image_u8.dim() != 3 or image_u8.shape[2] != 3 or image_u8.dtype != torch.uint8:
            raise ValueError("ViewEnsemble: an image is a uint8 (H0, W0, 3) tensor")
        _require_cuda(image_u8)
        logits, plan, frames = [], [], {}
        for scale, fx, fy in self.views:
            hw = working_frame(frame_hw, scale)
            if max(hw) > MAX_SIDE:
                raise ValueError(f"ViewEnsemble: a view of {hw[0]} x {hw[1]} at scale {scale} (sides up to {MAX_SIDE})")
            if hw not in frames:                       # the flips of one scale share the resized, normalised frame
                x = image_u8.unsqueeze(0)
                if tuple(x.shape[1:3]) != hw:
                    x = augment.resize_bilinear_u8(x, *hw)
                frames[hw] = augment.color_jitter_normalize_u8(x)[0]
            x = frames[hw]
            dims = [d for d, on in ((2, fx), (1, fy)) if on]
            z, tiles = self.predictor.blended_logits(torch.flip(x, dims) if dims else x)
            logits.append(z)
            plan.append({"scale": scale, "flip_x": bool(fx), "flip_y": bool(fy), "frame_size": list(hw), "tiling": tiles})
        return logits, plan

    def _flips(self):
        return [(fx, fy) for _s, fx, fy in self.views]

    def __call__(self, image_u8, frame_hw):
        logits, plan = self.view_logits(image_u8, frame_hw)
        labels, conf, agreement = merge_views(logits, self._flips(), frame_hw)
        return labels, conf, agreement, plan

    def merged_logits(self, image_u8, frame_hw):
        """The merged logits float32 (C, H, W) that ``__call__`` takes its labels and confidence from, for whoever needs
        more than the maximum: ``sheets.seg_confidence`` of them gives ``__call__``'s labels and confidence bit for bit."""
        logits, _plan = self.view_logits(image_u8, frame_hw)
        return merge_views(logits, self._flips(), frame_hw, merged=True, labels=False, conf=False, agreement=False)[3]
