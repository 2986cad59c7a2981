"""Prediction at an image's own resolution (no reference counterpart): a large frame is cut into overlapping tiles the
model runs at its trained size, and the tile logits are blended back into one label map and one confidence map on the
device (csrc/tiles.hip: unet_tile_gather, unet_tile_blend; restated by tests/_tiles_ref.py).

``plan_axis`` / ``plan_tiles`` place the tiles (plain integers: importable and testable without a GPU), ``gather_tiles``
and ``blend_tiles`` are the two launches, ``TiledPredictor`` strings them around a model.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from ._hipcall import _ptr, _require_cuda, _stream

MAX_TILES_AXIS = 64          # unet_tile_gather / unet_tile_blend: origins per axis
MAX_RAMP = 256               # unet_tile_blend: the largest ramp


def plan_axis(frame, tile, min_overlap):
    """The tile origins along one axis of ``frame`` pixels for tiles of ``L = min(tile, frame)``: ``[0]`` when one tile
    covers the axis, else the fewest tiles whose neighbours can overlap by at least ``min_overlap``,
    ``n = ceil((frame - min_overlap) / (L - min_overlap))``, spread evenly: origin i = ``i * (frame - L) // (n - 1)``
    (the first is 0, the last ``frame - L``, no step exceeds ``L - min_overlap``).  ValueError unless
    ``0 <= min_overlap < L``, or when more than 64 tiles would be needed."""
    frame, tile, min_overlap = int(frame), int(tile), int(min_overlap)
    if frame < 1 or tile < 1:
        raise ValueError(f"plan_axis: frame {frame} and tile {tile} must be positive")
    length = min(tile, frame)
    if not 0 <= min_overlap < length:
        raise ValueError(f"plan_axis: min_overlap {min_overlap} is not in 0..{length - 1} (tile {length})")
    if frame <= tile:
        return [0]
    step = length - min_overlap
    n = -(-(frame - min_overlap) // step)
    if n > MAX_TILES_AXIS:
        raise ValueError(f"plan_axis: {n} tiles of {length} over {frame} pixels (at most {MAX_TILES_AXIS} per axis)")
    return [i * (frame - length) // (n - 1) for i in range(n)]


def plan_tiles(frame_hw, tile_hw, min_overlap):
    """(th, tw, oy, ox): the tile size (no larger than the frame) and the origins of both axes (``plan_axis``)."""
    (h, w), (th, tw) = (int(v) for v in frame_hw), (int(v) for v in tile_hw)
    return min(th, h), min(tw, w), plan_axis(h, th, min_overlap), plan_axis(w, tw, min_overlap)


def default_ramp(origins, length):
    """The smallest overlap between neighbouring tiles of one axis, clipped to 1..256; 1 for a single tile."""
    origins = [int(o) for o in origins]
    if len(origins) < 2:
        return 1
    return max(1, min(MAX_RAMP, min(a + int(length) - b for a, b in zip(origins, origins[1:]))))


def _origins(oy, ox, what):
    out = []
    for name, o in (("oy", oy), ("ox", ox)):
        o = [int(v) for v in o]
        if not 1 <= len(o) <= MAX_TILES_AXIS:
            raise ValueError(f"{what}: {name} holds {len(o)} origins (1 to {MAX_TILES_AXIS})")
        out.append(((C.c_int32 * len(o))(*o), len(o)))
    return out


def gather_tiles(frame, th, tw, oy, ox):
    """The tiles (len(oy) * len(ox), C, th, tw) of a float32 DEVICE frame (C, H, W): tile ``i * len(ox) + j`` is
    ``frame[:, oy[i]:oy[i] + th, ox[j]:ox[j] + tw]``, bit for bit.  The origins of each axis must cover the frame (first
    0, last frame - tile, increasing, no gap wider than the tile).  One launch (unet_tile_gather); does not synchronise."""
    what = "gather_tiles"
    if not torch.is_tensor(frame) or frame.dim() != 3 or frame.dtype != torch.float32:
        raise ValueError(f"{what}: the frame is a float32 (C, H, W) tensor, got "
                         f"{(tuple(frame.shape), frame.dtype) if torch.is_tensor(frame) else type(frame).__name__}")
    c, h, w = frame.shape
    if min(c, h, w) < 1:
        raise ValueError(f"{what}: empty frame {tuple(frame.shape)}")
    (cy, ny), (cx, nx) = _origins(oy, ox, what)
    _require_cuda(frame)
    x = frame.detach().contiguous()
    th, tw = int(th), int(tw)
    if not (1 <= th <= h and 1 <= tw <= w):
        raise ValueError(f"{what}: tiles of {th} x {tw} in a frame of {h} x {w}")
    tiles = torch.empty((ny * nx, c, th, tw), dtype=torch.float32, device=x.device)
    L.check(L.lib().unet_tile_gather(_ptr(x), c, h, w, th, tw, cy, ny, cx, nx, _ptr(tiles), _stream()), "unet_tile_gather")
    return tiles


def blend_tiles(tile_logits, oy, ox, frame_hw, ramp=None, blended=False):
    """(labels, conf[, blended]) of a frame (H, W) from the float32 DEVICE logits (len(oy) * len(ox), C, th, tw) of its
    tiles, 2 <= C <= 8: labels uint8 (H, W), conf float32 (H, W), and with ``blended`` the blended logits float32
    (C, H, W).  A tile weighs ``q_y * q_x`` at a pixel, ``q(k) = min(k + 1, L - k, ramp)`` along each axis; a pixel under
    one tile takes its logits unchanged, and labels / conf follow by ``sheets.seg_confidence``'s rule.  ``ramp``: an int
    or (ramp_y, ramp_x), 1..256; None: per axis the smallest overlap between neighbouring tiles, clipped to 1..256 (1 for
    a single tile).  One launch (unet_tile_blend); does not synchronise."""
    what = "blend_tiles"
    if not torch.is_tensor(tile_logits) or tile_logits.dim() != 4 or tile_logits.dtype != torch.float32:
        raise ValueError(f"{what}: the tile logits are a float32 (T, C, th, tw) tensor, got "
                         f"{(tuple(tile_logits.shape), tile_logits.dtype) if torch.is_tensor(tile_logits) else type(tile_logits).__name__}")
    t, c, th, tw = tile_logits.shape
    (cy, ny), (cx, nx) = _origins(oy, ox, what)
    if t != ny * nx:
        raise ValueError(f"{what}: {t} tiles for {ny} x {nx} origins")
    h, w = (int(v) for v in frame_hw)
    if min(th, tw) < 1 or th > h or tw > w:
        raise ValueError(f"{what}: tiles of {th} x {tw} in a frame of {h} x {w}")
    if ramp is None:
        ramp_y, ramp_x = default_ramp(oy, th), default_ramp(ox, tw)
    else:
        ramp_y, ramp_x = (int(ramp), int(ramp)) if isinstance(ramp, int) else (int(v) for v in ramp)
    _require_cuda(tile_logits)
    z = tile_logits.detach().contiguous()
    labels = torch.empty((h, w), dtype=torch.uint8, device=z.device)
    conf = torch.empty((h, w), dtype=torch.float32, device=z.device)
    mixed = torch.empty((c, h, w), dtype=torch.float32, device=z.device) if blended else None
    L.check(L.lib().unet_tile_blend(_ptr(z), c, th, tw, cy, ny, cx, nx, h, w, ramp_y, ramp_x, _ptr(labels), _ptr(conf),
                                    _ptr(mixed), _stream()), "unet_tile_blend")
    return (labels, conf, mixed) if blended else (labels, conf)


class TiledPredictor:
    """``model`` over frames of any size: ``__call__(frame)`` takes a normalised float32 DEVICE frame (3, H, W) and returns
    (labels uint8 (H, W), conf float32 (H, W), plan), plan = ``{"tile": [th, tw], "origins_y", "origins_x", "ramp": [by,
    bx]}``.  The tiles are gathered in one launch, the model runs in eval mode under ``no_grad`` over chunks of
    ``batch_size`` tiles into one logits buffer, and one launch blends them.  One frame at a time: every image has its
    own size."""

    def __init__(self, model, tile_hw, min_overlap=64, batch_size=8):
        self.model = model
        self.tile_hw = (int(tile_hw[0]), int(tile_hw[1]))
        self.min_overlap, self.batch_size = int(min_overlap), int(batch_size)
        if min(self.tile_hw) < 1 or self.batch_size < 1:
            raise ValueError(f"TiledPredictor: tile {self.tile_hw} and batch_size {self.batch_size} must be positive")
        if not 0 <= self.min_overlap < min(self.tile_hw):
            raise ValueError(f"TiledPredictor: min_overlap {self.min_overlap} is not below the tile {self.tile_hw}")

    def tile_logits(self, tiles):
        """float32 logits (T, C, th, tw) of the tiles, ``batch_size`` at a time, in one buffer"""
        self.model.eval()
        out = None
        with torch.no_grad():
            for k in range(0, tiles.shape[0], self.batch_size):
                z = self.model(tiles[k:k + self.batch_size])
                if out is None:
                    out = torch.empty((tiles.shape[0],) + tuple(z.shape[1:]), dtype=torch.float32, device=tiles.device)
                out[k:k + z.shape[0]] = z
        return out

    def _planned_logits(self, frame):
        """(tile logits (T, C, th, tw), (H, W), plan) of a frame: the tiles placed, gathered and run through the model"""
        if not torch.is_tensor(frame) or frame.dim() != 3:
            raise ValueError("TiledPredictor: a frame is a (3, H, W) tensor")
        h, w = int(frame.shape[1]), int(frame.shape[2])
        # a frame side below min_overlap + 1 is one tile along that axis: the overlap only binds where tiles meet
        th, tw = min(self.tile_hw[0], h), min(self.tile_hw[1], w)
        oy = plan_axis(h, th, min(self.min_overlap, th - 1))
        ox = plan_axis(w, tw, min(self.min_overlap, tw - 1))
        plan = {"tile": [th, tw], "origins_y": oy, "origins_x": ox, "ramp": [default_ramp(oy, th), default_ramp(ox, tw)]}
        return self.tile_logits(gather_tiles(frame.float(), th, tw, oy, ox)), (h, w), plan

    def __call__(self, frame):
        logits, frame_hw, plan = self._planned_logits(frame)
        labels, conf = blend_tiles(logits, plan["origins_y"], plan["origins_x"], frame_hw, ramp=plan["ramp"])
        return labels, conf, plan

    def blended(self, frame):
        """(labels, conf, logits float32 (C, H, W), plan): ``__call__``'s results and the blended logits they are taken
        from, by the same plan and in the same single launch (``blend_tiles(..., blended=True)``), for whoever needs more
        than the maximum.  ``sheets.seg_confidence`` of the logits gives the labels and the confidence bit for bit."""
        logits, frame_hw, plan = self._planned_logits(frame)
        labels, conf, mixed = blend_tiles(logits, plan["origins_y"], plan["origins_x"], frame_hw, ramp=plan["ramp"],
                                          blended=True)
        return labels, conf, mixed, plan

    def blended_logits(self, frame):
        """(logits float32 (C, H, W), plan) of ``blended``"""
        _labels, _conf, mixed, plan = self.blended(frame)
        return mixed, plan
