"""Training crops at an image's own resolution (no reference counterpart: the reference trains on squeezed frames): affine
crops -- scale jitter, small rotation, flip -- cut on the device out of a batch of differently sized images in one launch
(csrc/crops.hip: unet_affine_crop_u8; restated by tests/_crops_ref.py).

``crop_matrix`` makes a crop's fixed-point matrix and ``CropSampler`` draws where the crops lie (plain host arithmetic:
importable and testable without a GPU), ``affine_crops_u8`` is the launch, ``GearCropPreprocess`` strings them into the
(images, masks) batches ``train_gear_crops`` trains on.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from ._hipcall import _ptr, _require_cuda, _stream

CROP_DTYPE = np.dtype([("image", "<i4"), ("a", "<i4", (6,)), ("reserved", "<i4")])          # struct unet_crop_desc
MAX_SCALE = 4.0
MAX_CROP_SIDE = 4096         # unet_affine_crop_u8: out_h, out_w
MAX_IMAGE_SIDE = 16384       # affine_crops_u8: with |a| <= 4 * 65536 every u, v stays far inside int64
MAX_COUNT = 65535            # unet_affine_crop_u8: images and crops per launch
IGNORE_INDEX = 255           # what a mask crop carries where the image crop carries fill
_MODES = {0: 0, 1: 1, "nearest": 0, "bilinear": 1}


def crop_matrix(cx, cy, scale, angle_deg, flip, out_h, out_w):
    """The six 16.16 fixed-point ints of the crop of ``out_h x out_w`` centred on source point (cx, cy) (pixel edges at
    integers, pixel centres at + 0.5): ``source = (cx, cy) + scale * R(angle) * diag(-1 if flip else 1, 1) * ((x + 0.5,
    y + 0.5) - (out_w / 2, out_h / 2))`` in float64, so ``scale > 1`` reads a larger source region (objects look smaller).
    a0 = f s cos, a1 = -s sin, a3 = f s sin, a4 = s cos, a2 = cx + a0 (0.5 - out_w / 2) + a1 (0.5 - out_h / 2), a5 likewise
    from cy, a3, a4; each fixed as floor(v * 65536 + 0.5), the half-pixel terms inside a2 / a5 (unet_flip_rotate_u8's
    convention).  ValueError unless 0 < scale <= 4 and every entry fits int32."""
    cx, cy, scale, angle_deg = float(cx), float(cy), float(scale), float(angle_deg)
    out_h, out_w = int(out_h), int(out_w)
    if not 0.0 < scale <= MAX_SCALE:
        raise ValueError(f"crop_matrix: scale {scale} is not in (0, {MAX_SCALE:g}]")
    if out_h < 1 or out_w < 1:
        raise ValueError(f"crop_matrix: a crop of {out_h} x {out_w}")
    f = -1.0 if flip else 1.0
    cos, sin = math.cos(math.radians(angle_deg)), math.sin(math.radians(angle_deg))
    a0, a1, a3, a4 = f * scale * cos, -scale * sin, f * scale * sin, scale * cos
    a2 = cx + a0 * (0.5 - out_w / 2) + a1 * (0.5 - out_h / 2)
    a5 = cy + a3 * (0.5 - out_w / 2) + a4 * (0.5 - out_h / 2)
    vals = (a0, a1, a2, a3, a4, a5)
    if not all(math.isfinite(v) for v in vals):
        raise ValueError("crop_matrix: the matrix is not finite")
    out = [int(math.floor(v * 65536.0 + 0.5)) for v in vals]
    if any(not -(1 << 31) <= v < (1 << 31) for v in out):
        raise ValueError("crop_matrix: the matrix is outside 16.16 fixed point")
    return out


def crop_table(descs) -> np.ndarray:
    """struct unet_crop_desc[K] from ``[(image, (a0, .., a5)), ...]`` (or such a table itself).  ValueError when an entry
    does not fit int32."""
    if isinstance(descs, np.ndarray) and descs.dtype == CROP_DTYPE:
        return np.ascontiguousarray(descs.reshape(-1))
    descs = list(descs)
    rec = np.zeros(len(descs), dtype=CROP_DTYPE)
    for k, (image, a) in enumerate(descs):
        a = [int(v) for v in a]
        if len(a) != 6 or any(not -(1 << 31) <= v < (1 << 31) for v in a + [int(image)]):
            raise ValueError(f"affine_crops_u8: crop {k} needs an image index and six int32 matrix entries")
        rec[k]["image"], rec[k]["a"] = int(image), a
    return rec


def _as_hwc(t, k, what):
    if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 3:
        got = (tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{what}: image {k} is not a uint8 [H, W, C] tensor, got {got}")
    return t


def affine_crops_u8(images, descs, out_hw, mode, fill, device=None):
    """uint8 [K, out_h, out_w, C] DEVICE crops of ``images``: a list of uint8 [H, W, C] tensors of any sizes, or a
    stacked [N, H, W, C] tensor, on the host or the device; C is 1 or 3 and the same for all, sides 1..16384.  ``descs``:
    ``[(image index, crop_matrix(...)), ...]`` (or ``crop_table`` of it), 1..65535 crops; ``out_hw`` sides 1..4096;
    ``mode`` 0 / "nearest" or 1 / "bilinear"; ``fill`` 0..255 is written where a crop leaves its image.  The arithmetic
    is the integer rule of csrc/crops.hip: a matrix that maps pixel centres to pixel centres copies bytes.

    Everything is checked before the device (ValueError).  The images are packed into one byte buffer; host images
    travel with the tables in ONE upload, device images are gathered on the device and only the tables are uploaded.
    ``device``: where to run; default: the device of the first image.  One launch (unet_affine_crop_u8); does not
    synchronise."""
    what = "affine_crops_u8"
    if torch.is_tensor(images):
        if images.dim() != 4:
            raise ValueError(f"{what}: a stacked batch is a uint8 [N, H, W, C] tensor, got {tuple(images.shape)}")
        items = list(images.unbind(0))
    else:
        items = list(images)
    if not 1 <= len(items) <= MAX_COUNT:
        raise ValueError(f"{what}: {len(items)} images (1 to {MAX_COUNT})")
    items = [_as_hwc(t, k, what) for k, t in enumerate(items)]
    c = int(items[0].shape[2])
    if c not in (1, 3):
        raise ValueError(f"{what}: C = {c} channels (1 or 3)")
    for k, t in enumerate(items):
        h, w, ck = (int(v) for v in t.shape)
        if ck != c:
            raise ValueError(f"{what}: image {k} has {ck} channels, image 0 has {c}")
        if not (1 <= h <= MAX_IMAGE_SIDE and 1 <= w <= MAX_IMAGE_SIDE):
            raise ValueError(f"{what}: image {k} is {h} x {w} (sides 1 to {MAX_IMAGE_SIDE})")
    table = crop_table(descs)
    if not 1 <= len(table) <= MAX_COUNT:
        raise ValueError(f"{what}: {len(table)} crops (1 to {MAX_COUNT})")
    bad = np.flatnonzero((table["image"] < 0) | (table["image"] >= len(items)))
    if len(bad):
        raise ValueError(f"{what}: crop {int(bad[0])} names image {int(table['image'][bad[0]])} of {len(items)}")
    out_h, out_w = (int(v) for v in out_hw)
    if not (1 <= out_h <= MAX_CROP_SIDE and 1 <= out_w <= MAX_CROP_SIDE):
        raise ValueError(f"{what}: crops of {out_h} x {out_w} (sides 1 to {MAX_CROP_SIDE})")
    if mode not in _MODES:
        raise ValueError(f"{what}: mode {mode!r} (0 / 'nearest' or 1 / 'bilinear')")
    fill = int(fill)
    if not 0 <= fill <= 255:
        raise ValueError(f"{what}: fill {fill} (0 to 255)")

    if device is None:
        device = items[0].device
    device = torch.device(device)
    if device.type != "cuda":
        _require_cuda(torch.empty(0, device=device))
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())

    n, k = len(items), len(table)
    sizes = np.asarray([(t.shape[0], t.shape[1]) for t in items], dtype=np.int64)
    nbytes = sizes[:, 0] * sizes[:, 1] * c
    offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    total = int(nbytes.sum())
    # the tables: src_offset int64 [n] | src_hw int32 [n][2] | desc [k] (32 bytes each), then -- from the host -- the images
    head = np.concatenate([offsets.view(np.uint8), sizes.astype(np.int32).reshape(-1).view(np.uint8),
                           table.view(np.uint8).reshape(-1)])
    head_bytes = 16 * n + 32 * k
    if all(not t.is_cuda for t in items):
        host = torch.empty(head_bytes + total, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        host[:head_bytes] = torch.from_numpy(head)
        torch.cat([t.reshape(-1) for t in items], out=host[head_bytes:])
        buf = host.to(device, non_blocking=True)
        tables, src = buf, buf[head_bytes:]
    else:
        tables = torch.from_numpy(head).to(device, non_blocking=True)
        src = torch.cat([t.to(device, non_blocking=True).reshape(-1) for t in items])
    base = tables.data_ptr()
    out = torch.empty((k, out_h, out_w, c), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        L.check(L.lib().unet_affine_crop_u8(_ptr(src), total, base, base + 8 * n, n, c, base + 16 * n, k, out_h, out_w,
                                            _MODES[mode], fill, _ptr(out), _stream()), "unet_affine_crop_u8")
    return out


# ---------------------------------------------------------------------------------------------------- where the crops lie
def footprint_half_extents(scale, angle_deg, crop_hw):
    """(ex, ey): half the width and height of the axis-aligned box around the source footprint of a crop of ``crop_hw``
    = (H, W): ex = s (|cos| W / 2 + |sin| H / 2), ey = s (|sin| W / 2 + |cos| H / 2)."""
    h, w = crop_hw
    cos, sin = abs(math.cos(math.radians(angle_deg))), abs(math.sin(math.radians(angle_deg)))
    return scale * (cos * w / 2 + sin * h / 2), scale * (sin * w / 2 + cos * h / 2)


def polygon_boxes(polys, n_images):
    """Per image the boxes (x0, y0, x1, y1) = (min x, min y, max x + 1, max y + 1) of its polygons, from the flat arrays
    of ``gear_dataset.flatten_polygons`` (which holds the known raw classes only)."""
    verts = np.asarray(polys["verts"], dtype=np.int64).reshape(-1, 2)
    offsets = np.asarray(polys["offsets"], dtype=np.int64).reshape(-1)
    boxes = [[] for _ in range(n_images)]
    for p, image in enumerate(np.asarray(polys["images"], dtype=np.int64).reshape(-1)):
        v = verts[offsets[p]:offsets[p + 1]]
        boxes[int(image)].append((float(v[:, 0].min()), float(v[:, 1].min()), float(v[:, 0].max() + 1),
                                  float(v[:, 1].max() + 1)))
    return boxes


class CropSampler:
    """Where training crops lie.  ``draw(sizes, boxes, crops_per_image)``: for every image ``crops_per_image`` crops, image
    by image, as a dict of per-crop lists ``image, cx, cy, scale, angle, flip, defect``.  Per crop, in this order, from
    one ``torch.Generator`` on the host: the flip (probability ``flip_p``), the angle (uniform in +-``degrees``), the
    scale (log-uniform in ``scale_range``), then the centre: with probability ``defect_fraction`` -- when the image has
    polygons -- uniform inside the bounding box of a uniformly chosen polygon (``defect`` True), otherwise uniform over
    the image.  The centre is then clamped per axis so that the crop's footprint stays inside the image: with
    ``footprint_half_extents`` (ex, ey), cx to [ex, w - ex] when w >= 2 ex, else cx = w / 2; cy likewise.  So fill
    appears only where an image is smaller than the footprint.  ``sizes`` = [(h, w)], ``boxes[i]`` = [(x0, y0, x1, y1)]."""

    def __init__(self, crop_hw, scale_range=(0.75, 1.5), degrees=10.0, flip_p=0.5, defect_fraction=0.5,
                 seed: Optional[int] = None):
        self.crop_hw = (int(crop_hw[0]), int(crop_hw[1]))
        self.scale_range = (float(scale_range[0]), float(scale_range[1]))
        self.degrees, self.flip_p, self.defect_fraction = float(degrees), float(flip_p), float(defect_fraction)
        if min(self.crop_hw) < 1 or max(self.crop_hw) > MAX_CROP_SIDE:
            raise ValueError(f"CropSampler: crops of {self.crop_hw} (sides 1 to {MAX_CROP_SIDE})")
        if not 0.0 < self.scale_range[0] <= self.scale_range[1] <= MAX_SCALE:
            raise ValueError(f"CropSampler: scale_range {self.scale_range} needs 0 < lo <= hi <= {MAX_SCALE:g}")
        if not (0.0 <= self.flip_p <= 1.0 and 0.0 <= self.defect_fraction <= 1.0):
            raise ValueError("CropSampler: flip_p and defect_fraction lie in 0..1")
        if not 0.0 <= self.degrees <= 180.0:
            raise ValueError("CropSampler: degrees lies in 0..180")
        self.gen = torch.Generator()
        if seed is not None:
            self.gen.manual_seed(int(seed))

    def _uniform(self, lo=0.0, hi=1.0):
        return lo + (hi - lo) * float(torch.rand(1, dtype=torch.float64, generator=self.gen))

    def draw(self, sizes, boxes, crops_per_image) -> dict:
        out = {key: [] for key in ("image", "cx", "cy", "scale", "angle", "flip", "defect")}
        log_lo, log_hi = math.log(self.scale_range[0]), math.log(self.scale_range[1])
        for i, (h, w) in enumerate(sizes):
            for _ in range(int(crops_per_image)):
                flip = self._uniform() < self.flip_p
                angle = self._uniform(-self.degrees, self.degrees)
                scale = min(max(math.exp(self._uniform(log_lo, log_hi)), self.scale_range[0]), self.scale_range[1])
                defect = bool(boxes[i]) and self._uniform() < self.defect_fraction
                if defect:
                    x0, y0, x1, y1 = boxes[i][int(torch.randint(len(boxes[i]), (1,), generator=self.gen))]
                else:
                    x0, y0, x1, y1 = 0.0, 0.0, float(w), float(h)
                cx, cy = self._uniform(x0, x1), self._uniform(y0, y1)
                ex, ey = footprint_half_extents(scale, angle, self.crop_hw)
                cx = min(max(cx, ex), w - ex) if w >= 2 * ex else w / 2
                cy = min(max(cy, ey), h - ey) if h >= 2 * ey else h / 2
                for key, v in zip(out, (i, cx, cy, scale, angle, flip, defect)):
                    out[key].append(v)
        return out

    def descs(self, params):
        """``[(image, crop_matrix(...))]`` of a drawn batch"""
        return [(i, crop_matrix(cx, cy, s, a, f, *self.crop_hw)) for i, cx, cy, s, a, f in
                zip(params["image"], params["cx"], params["cy"], params["scale"], params["angle"], params["flip"])]


# ---------------------------------------------------------------------------------------------------- Gear batches
def _subset_polygons(polys, keep):
    """The flat polygon arrays restricted to the images ``keep`` (ascending), renumbered 0..len(keep)-1."""
    offsets = np.asarray(polys["offsets"], dtype=np.int64).reshape(-1)
    images = np.asarray(polys["images"], dtype=np.int64).reshape(-1)
    verts = np.asarray(polys["verts"], dtype=np.int64).reshape(-1, 2)
    classes = np.asarray(polys["classes"], dtype=np.int64).reshape(-1)
    new_index = {int(i): j for j, i in enumerate(keep)}
    sel = [p for p in range(len(images)) if int(images[p]) in new_index]
    counts = [int(offsets[p + 1] - offsets[p]) for p in sel]
    return {"verts": (np.concatenate([verts[offsets[p]:offsets[p + 1]] for p in sel]) if sel
                      else np.zeros((0, 2), dtype=np.int64)),
            "offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
            "classes": classes[sel], "images": np.asarray([new_index[int(images[p])] for p in sel], dtype=np.int64)}


def full_resolution_masks(polys, sizes, device="cuda"):
    """The Gear class mask of every image at its own size, uint8 DEVICE [h, w] each: ``augment.polygon_masks_u8`` with
    the output size equal to the source size, once per distinct size of the batch."""
    from .augment import polygon_masks_u8
    sizes = [(int(h), int(w)) for h, w in sizes]
    groups = {}
    for i, hw in enumerate(sizes):
        groups.setdefault(hw, []).append(i)
    masks = [None] * len(sizes)
    for (h, w), idx in groups.items():
        sub = polys if len(groups) == 1 else _subset_polygons(polys, idx)
        m = polygon_masks_u8(sub, [(h, w)] * len(idx), h, w, device=device)
        for j, i in enumerate(idx):
            masks[i] = m[j]
    return masks


class GearCropPreprocess:
    """(images fp32 [K, 3, h, w], masks long [K, h, w]) on the device from a ``gear_dataset.collate_raw`` batch: K =
    ``crops_per_image`` crops of ``crop_hw`` per image, cut at the images' own resolution.  The class masks are made at
    full resolution (``full_resolution_masks``); images go through bilinear crops with fill 0, then
    ``augment.color_jitter_normalize_u8`` (Gear's ColorJitter(0.2, 0.2, 0.2, 0.1) when ``train``); masks go through
    nearest crops of the SAME matrices with fill 255, the loss' ignore value, so a mask is ignored exactly where its
    image is fill.  ``train=False`` draws centres alone: unit scale, no rotation, no flip, no ColorJitter.
    ``draw(sizes, polys)`` makes a batch's parameters (``CropSampler.draw`` plus the ColorJitter draws, one generator);
    pass them back as ``params`` to replay a batch (tests do)."""

    JITTER = ((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.1, 0.1))       # brightness, contrast, saturation, hue

    def __init__(self, crop_hw=(512, 512), train=False, crops_per_image=4, scale_range=(0.75, 1.5), degrees=10.0,
                 flip_p=0.5, defect_fraction=0.5, seed: Optional[int] = 0):
        self.train, self.crops_per_image = bool(train), int(crops_per_image)
        if self.crops_per_image < 1:
            raise ValueError("GearCropPreprocess: crops_per_image must be at least 1")
        if not self.train:
            scale_range, degrees, flip_p = (1.0, 1.0), 0.0, 0.0
        self.sampler = CropSampler(crop_hw, scale_range, degrees, flip_p, defect_fraction, seed)
        self.crop_hw = self.sampler.crop_hw

    def draw(self, sizes, polys) -> dict:
        p = self.sampler.draw(sizes, polygon_boxes(polys, len(sizes)), self.crops_per_image)
        if self.train:
            gen, k = self.sampler.gen, len(p["image"])
            p["orders"] = [torch.randperm(4, generator=gen).tolist() for _ in range(k)]
            for name, (lo, hi) in zip(("brightness", "contrast", "saturation", "hue"), self.JITTER):
                p[name] = torch.empty(k).uniform_(lo, hi, generator=gen).tolist()
        return p

    def __call__(self, images_u8, polys, sizes, device="cuda", params=None):
        from . import augment as A
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if params is None:
            params = self.draw(sizes, polys)
        descs = crop_table(self.sampler.descs(params))
        x = affine_crops_u8(images_u8, descs, self.crop_hw, L.CROP_BILINEAR, 0, device=device)
        jitter = None
        if self.train:
            jitter = A.jitter_table(params["orders"], params["brightness"], params["contrast"], params["saturation"],
                                    params["hue"])
        x = A.color_jitter_normalize_u8(x, jitter)
        masks = [m.unsqueeze(-1) for m in full_resolution_masks(polys, sizes, device=device)]
        m = affine_crops_u8(masks, descs, self.crop_hw, L.CROP_NEAREST, IGNORE_INDEX, device=device)
        return x, m[..., 0].long()
