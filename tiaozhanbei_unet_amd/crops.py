"""Training crops at an image's own resolution (no reference counterpart: the reference trains on squeezed frames): affine
crops -- scale jitter, small rotation, flip -- cut on the device out of a batch of differently sized images in one launch
(csrc/crops.hip: unet_affine_crop_u8; restated by tests/_crops_ref.py).

``crop_matrix`` makes a crop's fixed-point matrix and ``CropSampler`` draws where the crops lie (plain host arithmetic:
importable and testable without a GPU), ``affine_crops_u8`` is the launch, ``GearCropPreprocess`` strings them into the
(images, masks) batches ``train_gear_crops`` trains on.

Copy-paste augmentation (``train_gear_paste``; Ghiasi et al., CVPR 2021): ``paste_matrix`` and ``paste_dst_box`` place a
labelled defect of any image of the batch in a crop, ``PasteSampler`` draws which and where, and ``paste_crops_u8``
(csrc/paste.hip: unet_paste_crop_u8; restated by tests/_paste_ref.py) writes image crops and mask crops together, the
pastes applied on the way out, in one launch.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from ._hipcall import _ptr, _require_cuda, _stream

CROP_DTYPE = np.dtype([("image", "<i4"), ("a", "<i4", (6,)), ("reserved", "<i4")])          # struct unet_crop_desc
PASTE_DTYPE = np.dtype([("image", "<i4"), ("b", "<i4", (6,)), ("box", "<i4", (4,)), ("dst", "<i4", (4,)),
                        ("reserved", "<i4")])                                                # struct unet_paste_desc
MAX_PASTES = 8               # UNET_PASTE_MAX: pastes on one crop
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
    out_h, out_w = int(out_h), int(out_w)
    _check_scale("crop_matrix", scale)
    if out_h < 1 or out_w < 1:
        raise ValueError(f"crop_matrix: a crop of {out_h} x {out_w}")
    return _matrix("crop_matrix", cx, cy, scale, angle_deg, flip, out_w / 2, out_h / 2)


def _check_scale(who, scale):
    if not 0.0 < float(scale) <= MAX_SCALE:
        raise ValueError(f"{who}: scale {float(scale)} is not in (0, {MAX_SCALE:g}]")


def _matrix(who, cx, cy, scale, angle_deg, flip, px, py):
    """``crop_matrix``'s arithmetic with the crop point (px, py) that lands on (cx, cy)"""
    cx, cy, scale, angle_deg = float(cx), float(cy), float(scale), float(angle_deg)
    f = -1.0 if flip else 1.0
    cos, sin = math.cos(math.radians(angle_deg)), math.sin(math.radians(angle_deg))
    a0, a1, a3, a4 = f * scale * cos, -scale * sin, f * scale * sin, scale * cos
    a2 = cx + a0 * (0.5 - px) + a1 * (0.5 - py)
    a5 = cy + a3 * (0.5 - px) + a4 * (0.5 - py)
    vals = (a0, a1, a2, a3, a4, a5)
    if not all(math.isfinite(v) for v in vals):
        raise ValueError(f"{who}: the matrix is not finite")
    out = [int(math.floor(v * 65536.0 + 0.5)) for v in vals]
    if any(not -(1 << 31) <= v < (1 << 31) for v in out):
        raise ValueError(f"{who}: the matrix is outside 16.16 fixed point")
    return out


def paste_matrix(donor_cx, donor_cy, scale, angle_deg, flip, tx, ty):
    """The six 16.16 ints that take crop pixel (x, y) to the donor's source point, for a paste that puts donor point
    (donor_cx, donor_cy) on the crop point (tx, ty) (crop pixels, edges at integers): ``crop_matrix``'s formula with the
    crop centre (out_w / 2, out_h / 2) replaced by (tx, ty); its rounding and its refusals."""
    _check_scale("paste_matrix", scale)
    return _matrix("paste_matrix", donor_cx, donor_cy, scale, angle_deg, flip, float(tx), float(ty))


def paste_dst_box(b, box, out_h, out_w):
    """(x0, y0, x1, y1), half-open, crop pixels: a box that holds every pixel of an ``out_h x out_w`` crop at which the
    paste rule (include/unet_hip.h) can find a member of the donor ``box`` under matrix ``b``, through the nearest tap
    or a bilinear one; clamped to the crop; (0, 0, 0, 0) when there is none.  A member tap at column px needs
    (px - 1/2) 65536 <= u < (px + 3/2) 65536, so u lies in [(box x0 - 1/2) 65536, (box x1 + 1/2) 65536), v likewise: the
    pixels are those inside the parallelogram that ``b`` maps onto that rectangle, and the box is the one around its
    corners, found in exact integer arithmetic.  A singular matrix gives the whole crop."""
    b = [int(v) for v in b]
    bx0, by0, bx1, by1 = (int(v) for v in box)
    out_h, out_w = int(out_h), int(out_w)
    if bx0 >= bx1 or by0 >= by1:
        return (0, 0, 0, 0)
    det = b[0] * b[4] - b[1] * b[3]
    if det == 0:
        return (0, 0, out_w, out_h)
    xs, ys = [], []                                     # floors of the corners' x and y: // floors, whatever the signs
    for u in (bx0 * 65536 - 32768, bx1 * 65536 + 32768):
        for v in (by0 * 65536 - 32768, by1 * 65536 + 32768):
            du, dv = u - b[2], v - b[5]
            xs.append((b[4] * du - b[1] * dv) // det)
            ys.append((b[0] * dv - b[3] * du) // det)
    x0, x1 = max(min(xs), 0), min(max(xs) + 1, out_w)
    y0, y1 = max(min(ys), 0), min(max(ys) + 1, out_h)
    return (x0, y0, x1, y1) if x0 < x1 and y0 < y1 else (0, 0, 0, 0)


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
    items, c = _check_images(images, what, (1, 3))
    table = _check_crops(descs, len(items), out_hw, what)
    out_h, out_w = (int(v) for v in out_hw)
    if mode not in _MODES:
        raise ValueError(f"{what}: mode {mode!r} (0 / 'nearest' or 1 / 'bilinear')")
    fill = _check_byte(fill, "fill", what)
    device = _crop_device(device, items)

    n, k = len(items), len(table)
    offsets, sizes, total = _layout(items)
    # the tables: src_offset int64 [n] | src_hw int32 [n][2] | desc [k] (32 bytes each), then -- from the host -- the images
    head = np.concatenate([offsets.view(np.uint8), sizes.astype(np.int32).reshape(-1).view(np.uint8),
                           table.view(np.uint8).reshape(-1)])
    tables, (src,) = _upload(head, [items], device)
    base = tables.data_ptr()
    out = torch.empty((k, out_h, out_w, c), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        L.check(L.lib().unet_affine_crop_u8(_ptr(src), total, base, base + 8 * n, n, c, base + 16 * n, k, out_h, out_w,
                                            _MODES[mode], fill, _ptr(out), _stream()), "unet_affine_crop_u8")
    return out


def _check_images(images, what, channels):
    """the list of uint8 [H, W, C] tensors of ``images`` (a list or a stacked tensor) and C, or ValueError"""
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
    if c not in channels:
        raise ValueError(f"{what}: C = {c} channels ({' or '.join(str(v) for v in channels)})")
    for k, t in enumerate(items):
        h, w, ck = (int(v) for v in t.shape)
        if ck != c:
            raise ValueError(f"{what}: image {k} has {ck} channels, image 0 has {c}")
        if not (1 <= h <= MAX_IMAGE_SIDE and 1 <= w <= MAX_IMAGE_SIDE):
            raise ValueError(f"{what}: image {k} is {h} x {w} (sides 1 to {MAX_IMAGE_SIDE})")
    return items, c


def _check_crops(descs, n_images, out_hw, what):
    """``crop_table(descs)`` after the checks on the crops and their size"""
    table = crop_table(descs)
    if not 1 <= len(table) <= MAX_COUNT:
        raise ValueError(f"{what}: {len(table)} crops (1 to {MAX_COUNT})")
    bad = np.flatnonzero((table["image"] < 0) | (table["image"] >= n_images))
    if len(bad):
        raise ValueError(f"{what}: crop {int(bad[0])} names image {int(table['image'][bad[0]])} of {n_images}")
    out_h, out_w = (int(v) for v in out_hw)
    if not (1 <= out_h <= MAX_CROP_SIDE and 1 <= out_w <= MAX_CROP_SIDE):
        raise ValueError(f"{what}: crops of {out_h} x {out_w} (sides 1 to {MAX_CROP_SIDE})")
    return table


def _check_byte(value, name, what):
    if not 0 <= int(value) <= 255:
        raise ValueError(f"{what}: {name} {int(value)} (0 to 255)")
    return int(value)


def _crop_device(device, items):
    """the cuda device to run on (default: that of the first image); RuntimeError when it is no GPU"""
    if device is None:
        device = items[0].device
    device = torch.device(device)
    if device.type != "cuda":
        _require_cuda(torch.empty(0, device=device))
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _layout(items):
    """(byte offsets int64 [n], sizes int64 [n][2], total bytes) of tensors packed one after another"""
    sizes = np.asarray([(t.shape[0], t.shape[1]) for t in items], dtype=np.int64)
    nbytes = np.asarray([t.numel() for t in items], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    return offsets, sizes, int(nbytes.sum())


def _upload(head, groups, device):
    """The tables ``head`` (bytes) and each group of uint8 tensors, packed, on the device: (tables, [packed group]).  The
    groups whose tensors all live on the host travel behind the tables in ONE pinned upload; the tensors of any other
    group are gathered on the device."""
    head_bytes = len(head)
    on_host = [all(not t.is_cuda for t in g) for g in groups]
    total = sum(t.numel() for g, hst in zip(groups, on_host) if hst for t in g)
    if total:
        host = torch.empty(head_bytes + total, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        host[:head_bytes] = torch.from_numpy(head)
        torch.cat([t.reshape(-1) for g, hst in zip(groups, on_host) if hst for t in g], out=host[head_bytes:])
        tables = host.to(device, non_blocking=True)
    else:
        tables = torch.from_numpy(head).to(device, non_blocking=True)
    packed, at = [], head_bytes
    for g, hst in zip(groups, on_host):
        if hst:
            nbytes = sum(t.numel() for t in g)
            packed.append(tables[at:at + nbytes])
            at += nbytes
        else:
            packed.append(torch.cat([t.to(device, non_blocking=True).reshape(-1) for t in g]))
    return tables, packed


def paste_table(pastes, n_crops, n_images, out_hw, what="paste_crops_u8"):
    """(struct unet_paste_desc[P] sorted stably by crop with ``dst`` = ``paste_dst_box``, paste_start int32 [n_crops + 1])
    from ``[(crop, donor image, (b0, .., b5), (x0, y0, x1, y1)), ...]`` in any order.  ValueError when an entry does not
    fit, names a crop or an image that is not there, or a crop has more than ``MAX_PASTES``."""
    pastes = list(pastes)
    rows = []
    for j, entry in enumerate(pastes):
        try:
            crop, image, b, box = entry
            crop, image, b, box = int(crop), int(image), [int(v) for v in b], [int(v) for v in box]
        except (TypeError, ValueError):
            raise ValueError(f"{what}: paste {j} is not (crop, donor image, six matrix entries, a box of four)") from None
        if len(b) != 6 or len(box) != 4 or any(not -(1 << 31) <= v < (1 << 31) for v in b + box):
            raise ValueError(f"{what}: paste {j} needs six int32 matrix entries and an int32 box of four")
        if not 0 <= crop < n_crops:
            raise ValueError(f"{what}: paste {j} names crop {crop} of {n_crops}")
        if not 0 <= image < n_images:
            raise ValueError(f"{what}: paste {j} names donor image {image} of {n_images}")
        rows.append((crop, image, b, box))
    counts = np.bincount([r[0] for r in rows], minlength=n_crops) if rows else np.zeros(n_crops, dtype=np.int64)
    if len(rows) and counts.max() > MAX_PASTES:
        raise ValueError(f"{what}: crop {int(counts.argmax())} has {int(counts.max())} pastes (at most {MAX_PASTES})")
    rows.sort(key=lambda r: r[0])                       # stable: the order given holds within a crop
    flat = [[image, *b, *box, *paste_dst_box(b, box, out_hw[0], out_hw[1]), 0] for _crop, image, b, box in rows]
    rec = np.asarray(flat, dtype="<i4").reshape(-1, 16).view(PASTE_DTYPE).reshape(-1)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return rec, start


def paste_crops_u8(images, masks, descs, pastes, out_hw, fill=0, ignore=IGNORE_INDEX, device=None):
    """(uint8 [K, out_h, out_w, 3], uint8 [K, out_h, out_w]) DEVICE: the bilinear crops of ``images`` and the nearest crops
    of their ``masks`` that two ``affine_crops_u8`` calls would cut, with ``pastes`` applied on the way out, in ONE launch
    (unet_paste_crop_u8, csrc/paste.hip; the rule stands in include/unet_hip.h).  ``images``: as for ``affine_crops_u8``,
    3 channels; ``masks``: one uint8 [H, W] tensor per image, of the image's size; ``descs``, ``out_hw``, ``fill`` as
    there; ``ignore`` 0..255 is the label written where a crop leaves its image, and a donor label that no paste carries.
    ``pastes``: ``[(crop, donor image, paste_matrix(...), (x0, y0, x1, y1) donor box), ...]`` in any order, at most 8 on a
    crop, a later one on top (``paste_table``); may be empty.

    Everything is checked before the device (ValueError).  Host images and host masks travel with all tables in ONE
    upload, device ones are gathered on the device.  Does not synchronise."""
    what = "paste_crops_u8"
    items, _c = _check_images(images, what, (3,))
    n = len(items)
    mask_items = list(masks.unbind(0)) if torch.is_tensor(masks) else list(masks)
    if len(mask_items) != n:
        raise ValueError(f"{what}: {len(mask_items)} masks for {n} images")
    for i, (m, t) in enumerate(zip(mask_items, items)):
        if not torch.is_tensor(m) or m.dtype != torch.uint8 or tuple(m.shape) != tuple(t.shape[:2]):
            got = (tuple(m.shape), m.dtype) if torch.is_tensor(m) else type(m).__name__
            raise ValueError(f"{what}: mask {i} is not a uint8 {list(t.shape[:2])} tensor, got {got}")
    table = _check_crops(descs, n, out_hw, what)
    out_h, out_w = (int(v) for v in out_hw)
    fill, ignore = _check_byte(fill, "fill", what), _check_byte(ignore, "ignore", what)
    k = len(table)
    rec, start = paste_table(pastes, k, n, (out_h, out_w), what)
    device = _crop_device(device, items)

    offsets, sizes, total = _layout(items)
    mask_offsets, _sizes, mask_total = _layout(mask_items)
    # the tables: src_offset int64 [n] | mask_offset int64 [n] | src_hw int32 [n][2] | desc [k] (32 bytes each) | paste [p]
    # (64 bytes each) | paste_start int32 [k + 1], then -- from the host -- the images and the masks
    head = np.concatenate([offsets.view(np.uint8), mask_offsets.view(np.uint8),
                           sizes.astype(np.int32).reshape(-1).view(np.uint8), table.view(np.uint8).reshape(-1),
                           rec.view(np.uint8).reshape(-1), start.view(np.uint8)])
    tables, (src, msk) = _upload(head, [items, mask_items], device)
    base = tables.data_ptr()
    at_desc = 24 * n
    at_paste = at_desc + 32 * k
    at_start = at_paste + 64 * len(rec)
    out = torch.empty((k, out_h, out_w, 3), dtype=torch.uint8, device=device)
    out_mask = torch.empty((k, out_h, out_w), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        L.check(L.lib().unet_paste_crop_u8(_ptr(src), total, base, base + 16 * n, n, _ptr(msk), mask_total, base + 8 * n,
                                           base + at_desc, k, base + at_start, base + at_paste if len(rec) else None,
                                           len(rec), out_h, out_w, fill, ignore, _ptr(out), _ptr(out_mask), _stream()),
                "unet_paste_crop_u8")
    return out, out_mask


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


class PasteSampler:
    """Which labelled defects are pasted into which crops (copy-paste augmentation).  ``draw(crop_params, polys, sizes)``:
    for the crops of ``CropSampler.draw`` and the batch's flat polygon arrays, a list of pastes, each a tuple ``(crop,
    donor image, raw class, donor cx, donor cy, scale, angle, flip, tx, ty, box)``.  Plain host arithmetic from the
    sampler's OWN ``torch.Generator`` (``seed + 1``), so the crops of a run are those it would draw without pasting.
    Per crop, in this order: with probability ``paste_p`` the crop takes pastes, n uniform in 1..``max_pastes``; per
    paste a raw class uniform among the classes the batch's polygons hold, then a polygon uniform within that class
    (rare classes are pasted as often as common ones), the flip (p = 0.5), the angle (uniform in +-``degrees``), the
    scale (the crop's own times a log-uniform factor in ``scale_range``, clamped into (0, 4]), the target (tx, ty)
    (uniform over the crop).  The donor centre is the centre of the polygon's box, ``box`` that box
    (``polygon_boxes``).  A batch without polygons draws nothing.  ``counts`` sums the pastes drawn per raw class."""

    def __init__(self, crop_hw, paste_p=0.5, max_pastes=2, scale_range=(0.75, 1.33), degrees=180.0,
                 seed: Optional[int] = None):
        self.crop_hw = (int(crop_hw[0]), int(crop_hw[1]))
        self.paste_p, self.max_pastes = float(paste_p), int(max_pastes)
        self.scale_range, self.degrees = (float(scale_range[0]), float(scale_range[1])), float(degrees)
        if min(self.crop_hw) < 1 or max(self.crop_hw) > MAX_CROP_SIDE:
            raise ValueError(f"PasteSampler: crops of {self.crop_hw} (sides 1 to {MAX_CROP_SIDE})")
        if not 0.0 <= self.paste_p <= 1.0:
            raise ValueError("PasteSampler: paste_p lies in 0..1")
        if not 1 <= self.max_pastes <= MAX_PASTES:
            raise ValueError(f"PasteSampler: max_pastes lies in 1..{MAX_PASTES}")
        if not 0.0 < self.scale_range[0] <= self.scale_range[1] <= MAX_SCALE:
            raise ValueError(f"PasteSampler: scale_range {self.scale_range} needs 0 < lo <= hi <= {MAX_SCALE:g}")
        if not 0.0 <= self.degrees <= 180.0:
            raise ValueError("PasteSampler: degrees lies in 0..180")
        self.gen = torch.Generator()
        if seed is not None:
            self.gen.manual_seed(int(seed) + 1)
        self.counts = {}

    def _uniform(self, lo=0.0, hi=1.0):
        return lo + (hi - lo) * float(torch.rand(1, dtype=torch.float64, generator=self.gen))

    def _randint(self, n):
        return int(torch.randint(n, (1,), generator=self.gen))

    def draw(self, crop_params, polys, sizes) -> list:
        images = np.asarray(polys["images"], dtype=np.int64).reshape(-1)
        classes = np.asarray(polys["classes"], dtype=np.int64).reshape(-1)
        if len(images) == 0:
            return []
        boxes, seen, by_class = polygon_boxes(polys, len(sizes)), {}, {}
        for p, (image, cls) in enumerate(zip(images.tolist(), classes.tolist())):
            box = tuple(int(v) for v in boxes[image][seen.get(image, 0)])
            seen[image] = seen.get(image, 0) + 1
            by_class.setdefault(cls, []).append((image, box))
        present = sorted(by_class)
        log_lo, log_hi = math.log(self.scale_range[0]), math.log(self.scale_range[1])
        out = []
        for k, crop_scale in enumerate(crop_params["scale"]):
            if not self._uniform() < self.paste_p:
                continue
            for _ in range(1 + self._randint(self.max_pastes)):
                cls = present[self._randint(len(present))]
                image, box = by_class[cls][self._randint(len(by_class[cls]))]
                flip = self._uniform() < 0.5
                angle = self._uniform(-self.degrees, self.degrees)
                scale = min(float(crop_scale) * math.exp(self._uniform(log_lo, log_hi)), MAX_SCALE)
                tx, ty = self._uniform(0.0, self.crop_hw[1]), self._uniform(0.0, self.crop_hw[0])
                out.append((k, image, cls, (box[0] + box[2]) / 2, (box[1] + box[3]) / 2, scale, angle, flip, tx, ty, box))
                self.counts[cls] = self.counts.get(cls, 0) + 1
        return out

    def report(self) -> str:
        """one line on the pastes drawn per class since the last report (host counts), which it clears"""
        from .gear_dataset import CLASS_ORDER
        counts, self.counts = self.counts, {}
        per_class = ", ".join(f"{name} {counts.get(raw, 0)}" for raw, name in enumerate(CLASS_ORDER))
        return f"Pastes drawn: {sum(counts.values())} ({per_class})"

    @staticmethod
    def table(pastes):
        """``[(crop, donor image, paste_matrix(...), box)]`` of drawn pastes, as ``paste_crops_u8`` takes them"""
        return [(k, image, paste_matrix(cx, cy, s, a, f, tx, ty), box)
                for k, image, _cls, cx, cy, s, a, f, tx, ty, box in pastes]


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
    pass them back as ``params`` to replay a batch (tests do).
    ``paste``: a ``PasteSampler`` for copy-paste augmentation, or None.  With None the code path, the generator draws and
    the launches are the ones above.  With a sampler ``draw`` adds ``params["pastes"]`` (from the sampler's own
    generator), and the image and mask crops come out of ONE ``paste_crops_u8`` launch in place of the two crop launches,
    ColorJitter running on the composite, so donor and base are jittered alike."""

    JITTER = ((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.1, 0.1))       # brightness, contrast, saturation, hue

    def __init__(self, crop_hw=(512, 512), train=False, crops_per_image=4, scale_range=(0.75, 1.5), degrees=10.0,
                 flip_p=0.5, defect_fraction=0.5, seed: Optional[int] = 0, paste: Optional[PasteSampler] = None):
        self.train, self.crops_per_image = bool(train), int(crops_per_image)
        if self.crops_per_image < 1:
            raise ValueError("GearCropPreprocess: crops_per_image must be at least 1")
        if not self.train:
            scale_range, degrees, flip_p = (1.0, 1.0), 0.0, 0.0
        self.sampler = CropSampler(crop_hw, scale_range, degrees, flip_p, defect_fraction, seed)
        self.crop_hw = self.sampler.crop_hw
        if paste is not None and paste.crop_hw != self.crop_hw:
            raise ValueError(f"GearCropPreprocess: the paste sampler draws for crops of {paste.crop_hw}, not {self.crop_hw}")
        self.paste = paste

    def draw(self, sizes, polys) -> dict:
        p = self.sampler.draw(sizes, polygon_boxes(polys, len(sizes)), self.crops_per_image)
        if self.train:
            gen, k = self.sampler.gen, len(p["image"])
            p["orders"] = [torch.randperm(4, generator=gen).tolist() for _ in range(k)]
            for name, (lo, hi) in zip(("brightness", "contrast", "saturation", "hue"), self.JITTER):
                p[name] = torch.empty(k).uniform_(lo, hi, generator=gen).tolist()
        if self.paste is not None:
            p["pastes"] = self.paste.draw(p, polys, sizes)
        return p

    def __call__(self, images_u8, polys, sizes, device="cuda", params=None):
        from . import augment as A
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if params is None:
            params = self.draw(sizes, polys)
        descs = crop_table(self.sampler.descs(params))
        jitter = None
        if self.train:
            jitter = A.jitter_table(params["orders"], params["brightness"], params["contrast"], params["saturation"],
                                    params["hue"])
        if self.paste is not None:
            x, m = paste_crops_u8(images_u8, full_resolution_masks(polys, sizes, device=device), descs,
                                  self.paste.table(params["pastes"]), self.crop_hw, 0, IGNORE_INDEX, device=device)
            return A.color_jitter_normalize_u8(x, jitter), m.long()
        x = affine_crops_u8(images_u8, descs, self.crop_hw, L.CROP_BILINEAR, 0, device=device)
        x = A.color_jitter_normalize_u8(x, jitter)
        masks = [m.unsqueeze(-1) for m in full_resolution_masks(polys, sizes, device=device)]
        m = affine_crops_u8(masks, descs, self.crop_hw, L.CROP_NEAREST, IGNORE_INDEX, device=device)
        return x, m[..., 0].long()
