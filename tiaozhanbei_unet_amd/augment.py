"""The loaders' image transform on the GPU: host side of csrc/augment.hip.

The reference builds its transforms from torchvision on PIL images (/root/reference/src/dataset.py:130-154,
src/kolektorsdd_dataset.py:133-155):

    Resize -> RandomHorizontalFlip(0.5) -> RandomRotation(10 | 5) -> ColorJitter(0.1, 0.1, 0.1, 0.05) -> ToTensor -> Normalize

Every one of those ends in a Pillow C kernel; libunet_hip restates that arithmetic on the device (bit-exact against PIL,
tests/golden/aug_*.npz), so loader workers only DECODE and ship the raw uint8 image.  What stays on the host is what is
host work in the reference too: the random draws (same distributions, same per-sample order as torchvision's
``get_params``; the RNG *stream* is this module's own generator -- torchvision is not installable here, so the stream
itself is "parity unpinned") and the parameter set-up PIL does in Python (``Image.rotate``'s matrix) or per axis
(the resampling tables, computed by the library's host functions).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .ops import _ptr, _require_cuda, _stream

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)

JITTER_DTYPE = np.dtype([("order", "<i4", (4,)), ("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4"),
                         ("hue_shift", "<i4")])          # struct unet_jitter_desc

_tables = {}


def _axis_tables(kind: str, in_size: int, out_size: int, device):
    """PIL's per-axis tables in device memory, cached per (kind, sizes, device): ('bilinear' -> bounds, kk, ksize),
    ('nearest' -> idx)."""
    key = (kind, in_size, out_size, device.index)
    hit = _tables.get(key)
    if hit is not None:
        return hit
    lib = L.lib()
    if kind == "bilinear":
        ksize = lib.unet_resize_bilinear_ksize(in_size, out_size)
        bounds = np.zeros((out_size, 2), dtype=np.int32)
        kk = np.zeros((out_size, ksize), dtype=np.int32)
        L.check(lib.unet_resize_bilinear_coeffs(in_size, out_size, bounds.ctypes.data_as(C.c_void_p),
                                                kk.ctypes.data_as(C.c_void_p)), "unet_resize_bilinear_coeffs")
        hit = (torch.from_numpy(bounds).to(device), torch.from_numpy(kk).to(device), ksize)
    else:
        idx = np.zeros(out_size, dtype=np.int32)
        L.check(lib.unet_resize_nearest_index(in_size, out_size, idx.ctypes.data_as(C.c_void_p)),
                "unet_resize_nearest_index")
        hit = (torch.from_numpy(idx).to(device),)
    _tables[key] = hit
    return hit


def _check_u8(images: torch.Tensor, what: str):
    _require_cuda(images)
    if images.dtype != torch.uint8 or images.dim() != 4:
        raise ValueError(f"{what} expects a uint8 [N, H, W, C] device tensor")
    return images.contiguous()


def resize_bilinear_u8(images: torch.Tensor, out_h: int, out_w: int) -> torch.Tensor:
    """``transforms.Resize((out_h, out_w))`` of PIL images = ``Image.resize((out_w, out_h), BILINEAR)`` for a batch of
    equally sized uint8 [N, H, W, C] images (C = 1 or 3) on the device (unet_resize_bilinear_u8)."""
    images = _check_u8(images, "resize_bilinear_u8")
    n, h, w, c = images.shape
    dev = images.device
    out = torch.empty((n, out_h, out_w, c), dtype=torch.uint8, device=dev)
    xb = xk = yb = yk = None
    xs = ys = 0
    if out_w != w:
        xb, xk, xs = _axis_tables("bilinear", w, out_w, dev)
    if out_h != h:
        yb, yk, ys = _axis_tables("bilinear", h, out_h, dev)
    tmp = torch.empty((n, h, out_w, c), dtype=torch.uint8, device=dev) if (out_w != w and out_h != h) else None
    L.check(L.lib().unet_resize_bilinear_u8(_ptr(images), n, h, w, c, out_h, out_w, _ptr(xb), _ptr(xk), xs, _ptr(yb), _ptr(yk),
                                            ys, _ptr(tmp), _ptr(out), _stream()), "unet_resize_bilinear_u8")
    return out


def resize_nearest_u8(images: torch.Tensor, out_h: int, out_w: int) -> torch.Tensor:
    """``Image.resize((out_w, out_h), NEAREST)`` (the Kolektor mask transform, src/kolektorsdd_dataset.py:116-117,147-150)."""
    images = _check_u8(images, "resize_nearest_u8")
    n, h, w, c = images.shape
    dev = images.device
    (yi,) = _axis_tables("nearest", h, out_h, dev)
    (xi,) = _axis_tables("nearest", w, out_w, dev)
    out = torch.empty((n, out_h, out_w, c), dtype=torch.uint8, device=dev)
    L.check(L.lib().unet_resize_nearest_u8(_ptr(images), n, h, w, c, out_h, out_w, _ptr(yi), _ptr(xi), _ptr(out), _stream()),
            "unet_resize_nearest_u8")
    return out


def rotation_matrix_fixed(w: int, h: int, angle: float) -> List[int]:
    """The six 16.16 fixed-point coefficients Pillow's ``Image.rotate(angle, NEAREST)`` ends up with: the Python half
    (Image.py: angle % 360, cos / sin rounded to 15 decimals, centre (w/2, h/2)) and the C half (Geometry.c affine_fixed:
    FIX(v) = floor(v * 65536 + 0.5), half-pixel terms folded into the translation)."""
    angle = angle % 360.0
    cx, cy = w / 2, h / 2
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy

    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))

    out = [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]
    if any(abs(v) >= 1 << 31 for v in out):
        raise ValueError("rotation matrix outside 16.16 fixed point")
    return out


def flip_rotate_u8(images: torch.Tensor, flips=None, angles: Optional[Sequence[float]] = None) -> torch.Tensor:
    """RandomHorizontalFlip then RandomRotation (``Image.rotate(angle, NEAREST, expand=False)``, fill 0) with per-image
    flip flags / angles in degrees (unet_flip_rotate_u8)."""
    images = _check_u8(images, "flip_rotate_u8")
    n, h, w, c = images.shape
    dev = images.device
    fl = None if flips is None else torch.as_tensor(flips).to(device=dev, dtype=torch.uint8).contiguous()
    mats = None
    if angles is not None:
        mats = torch.tensor([rotation_matrix_fixed(w, h, float(a)) for a in angles], dtype=torch.int32).to(dev)
    out = torch.empty_like(images)
    L.check(L.lib().unet_flip_rotate_u8(_ptr(images), n, h, w, c, _ptr(fl), _ptr(mats), _ptr(out), _stream()),
            "unet_flip_rotate_u8")
    return out


def jitter_table(orders, brightness, contrast, saturation, hue) -> np.ndarray:
    """struct unet_jitter_desc[n] from torchvision-style parameters: ``orders[n]`` = permutation of (0 brightness, 1
    contrast, 2 saturation, 3 hue; -1 skips a slot), three enhancement factors and the hue factor in [-0.5, 0.5]
    (``np.uint8(hue_factor * 255)``: truncated toward zero, wrapped to a byte -- torchvision's adjust_hue)."""
    n = len(orders)
    rec = np.zeros(n, dtype=JITTER_DTYPE)
    for i in range(n):
        rec[i]["order"] = np.asarray(orders[i], dtype=np.int32)
        rec[i]["brightness"], rec[i]["contrast"], rec[i]["saturation"] = brightness[i], contrast[i], saturation[i]
        rec[i]["hue_shift"] = int(float(hue[i]) * 255) & 255
    return rec


def color_jitter_normalize_u8(images: torch.Tensor, jitter: Optional[np.ndarray] = None, mean=MEAN, std=STD) -> torch.Tensor:
    """ColorJitter (optional: ``jitter`` = jitter_table(...)) + ToTensor + Normalize: uint8 [N, H, W, 3] -> fp32 NCHW."""
    images = _check_u8(images, "color_jitter_normalize_u8")
    n, h, w, c = images.shape
    if c != 3:
        raise ValueError("color_jitter_normalize_u8 expects RGB images")
    dev = images.device
    out = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)
    lib = L.lib()
    desc = ws = None
    if jitter is not None:
        if jitter.dtype != JITTER_DTYPE or jitter.shape != (n,):
            raise ValueError("jitter: expected jitter_table(...) of the batch size")
        desc = torch.from_numpy(jitter.view(np.uint8).reshape(n, -1).copy()).to(dev)
        ws = torch.empty(lib.unet_color_jitter_workspace(n), dtype=torch.uint8, device=dev)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s_ = (C.c_float * 3)(*[float(v) for v in std])
    L.check(lib.unet_color_jitter_normalize_u8(_ptr(images), n, h, w, _ptr(desc), m, s_, _ptr(out), _ptr(ws),
                                               0 if ws is None else ws.numel(), _stream()), "unet_color_jitter_normalize_u8")
    return out


def _resize_any(images, out_h, out_w, device, nearest=False):
    """A stacked [N, H, W, C] tensor or a list of differently sized [H, W, C] tensors -> [N, out_h, out_w, C] on the device."""
    fn = resize_nearest_u8 if nearest else resize_bilinear_u8
    if isinstance(images, torch.Tensor):
        return fn(images.to(device, non_blocking=True), out_h, out_w)
    items = [t if t.dim() == 3 else t.unsqueeze(-1) for t in images]
    out = torch.empty((len(items), out_h, out_w, items[0].shape[-1]), dtype=torch.uint8, device=device)
    groups = {}
    for i, t in enumerate(items):
        groups.setdefault(tuple(t.shape), []).append(i)
    for idx in groups.values():
        batch = torch.stack([items[i] for i in idx]).to(device, non_blocking=True)
        out[torch.as_tensor(idx, device=device)] = fn(batch, out_h, out_w)
    return out


class DeviceTransform:
    """``get_transforms(image_size, is_train)[0]`` of the reference (src/dataset.py:130-146; ``degrees=5`` gives
    src/kolektorsdd_dataset.py:133-150) for batches of decoded uint8 RGB images, on the GPU.

    ``__call__(images)`` -> normalised fp32 NCHW; ``images`` is a stacked uint8 [N, H, W, 3] tensor or a list of
    [H, W, 3] tensors of any sizes (host or device).  ``draw(n)`` makes the per-sample random parameters (the same
    distributions and per-sample order as torchvision: flip, angle, then ColorJitter's permutation and four factors);
    pass them back as ``params`` to replay a batch (tests do)."""

    def __init__(self, size, train: bool, degrees=10.0, brightness=0.1, contrast=0.1, saturation=0.1, hue=0.05,
                 flip_p=0.5, seed: Optional[int] = None, mean=MEAN, std=STD):
        self.size = (size, size) if isinstance(size, int) else tuple(size)
        self.train = bool(train)
        self.degrees, self.flip_p = float(degrees), float(flip_p)
        self.ranges = ((max(0.0, 1 - brightness), 1 + brightness), (max(0.0, 1 - contrast), 1 + contrast),
                       (max(0.0, 1 - saturation), 1 + saturation), (-hue, hue))
        self.mean, self.std = tuple(mean), tuple(std)
        self.gen = torch.Generator()
        if seed is not None:
            self.gen.manual_seed(int(seed))

    def draw(self, n: int) -> dict:
        flips, angles, orders, fac = [], [], [], [[], [], [], []]
        for _ in range(n):
            flips.append(bool(torch.rand(1, generator=self.gen) < self.flip_p))
            angles.append(float(torch.empty(1).uniform_(-self.degrees, self.degrees, generator=self.gen)))
            orders.append(torch.randperm(4, generator=self.gen).tolist())
            for k, (lo, hi) in enumerate(self.ranges):
                fac[k].append(float(torch.empty(1).uniform_(lo, hi, generator=self.gen)))
        return {"flips": flips, "angles": angles, "orders": orders, "brightness": fac[0], "contrast": fac[1],
                "saturation": fac[2], "hue": fac[3]}

    def __call__(self, images, params: Optional[dict] = None, device="cuda") -> torch.Tensor:
        device = torch.device(device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        x = _resize_any(images, self.size[0], self.size[1], device)
        jitter = None
        if self.train:
            p = params if params is not None else self.draw(x.shape[0])
            x = flip_rotate_u8(x, p["flips"], p["angles"])
            jitter = jitter_table(p["orders"], p["brightness"], p["contrast"], p["saturation"], p["hue"])
        return color_jitter_normalize_u8(x, jitter, self.mean, self.std)

    def masks(self, masks, device="cuda") -> torch.Tensor:
        """``get_transforms(...)[1]`` (src/dataset.py:148-151): Resize (bilinear) + ToTensor of the {0, 1} uint8 masks
        -> fp32 [N, 1, H, W] (values k/255: the reference's mask quirk, reproduced by feeding the same data)."""
        device = torch.device(device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        m = _resize_any(masks, self.size[0], self.size[1], device)
        return (m.permute(0, 3, 1, 2).float() / 255.0).contiguous()


POLY_MAX_VERTICES = 512      # unet_polygon_mask_u8: crossings of one polygon on one scan line live in LDS
POLY_MAX_WIDTH = 4096        # ... and so does the row of class bits


def _nearest_tables(sizes, out_h, out_w, device):
    """Per-image NEAREST index tables [N, out_h] / [N, out_w] (unet_resize_nearest_index) for a list of (h, w)."""
    ys = [_axis_tables("nearest", h, out_h, device)[0] for h, _ in sizes]
    xs = [_axis_tables("nearest", w, out_w, device)[0] for _, w in sizes]
    return torch.stack(ys).contiguous(), torch.stack(xs).contiguous()


def _check_polygons(what, polys, sizes):
    """The flat polygon arrays of ``gear_dataset.flatten_polygons`` as int64 numpy arrays, refused with ValueError when
    they do not describe ``len(sizes)`` images the polygon kernels can take: (verts, offsets, classes, images, counts)."""
    n = len(sizes)
    verts = np.ascontiguousarray(np.asarray(polys["verts"], dtype=np.int64).reshape(-1, 2))
    offsets = np.asarray(polys["offsets"], dtype=np.int64).reshape(-1)
    classes = np.asarray(polys["classes"], dtype=np.int64).reshape(-1)
    images = np.asarray(polys["images"], dtype=np.int64).reshape(-1)
    p = len(classes)
    if len(offsets) != p + 1 or len(images) != p or offsets[0] != 0 or offsets[-1] != len(verts):
        raise ValueError(f"{what}: offsets / classes / images do not describe the vertex array")
    counts = np.diff(offsets)
    if p and (counts.min() < 3 or counts.max() > POLY_MAX_VERTICES):
        bad = int(np.argmax((counts < 3) | (counts > POLY_MAX_VERTICES)))
        raise ValueError(f"{what}: polygon {bad} of image {int(images[bad])} has {int(counts[bad])} vertices; "
                         f"every polygon needs 3..{POLY_MAX_VERTICES}")
    if p and (np.any(np.diff(images) < 0) or images.min() < 0 or images.max() >= n):
        raise ValueError(f"{what}: image indices must be non-decreasing and inside the batch")
    if verts.size and np.abs(verts).max() >= (1 << 24):
        raise ValueError(f"{what}: coordinates must stay below 2^24 in magnitude (exact in float32)")
    if any(h <= 0 or w <= 0 or h >= (1 << 24) or w >= (1 << 24) for h, w in sizes):
        raise ValueError(f"{what}: bad source size")
    return verts, offsets, classes, images, counts


def polygon_masks_u8(polys, src_sizes, out_h: int, out_w: int, device="cuda") -> torch.Tensor:
    """Gear class masks of a batch, on the device (unet_polygon_mask_u8): ``GearDataset._create_mask_from_labelme`` of the
    reference (src/gear_dataset.py:112-201) followed by ``Image.resize((out_w, out_h), NEAREST)``, without a
    full-resolution mask ever existing.  Equal to the reference on every fixture case except polygons that revisit a
    vertex, where a few pixels on that vertex's row can differ (csrc/polygon.hip, "Known divergence").  ``polys`` = the flat arrays ``gear_dataset.collate_raw`` builds: ``verts`` int32
    [V, 2] pixel (x, y), ``offsets`` [P + 1], ``classes`` [P] raw class ids, ``images`` [P] (non-decreasing);
    ``src_sizes`` = [(h, w)] per image.  Output sizes equal to a source size give that image's full-resolution mask.
    Returns uint8 [N, out_h, out_w]."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    sizes = [(int(h), int(w)) for h, w in src_sizes]
    n = len(sizes)
    if n == 0 or out_h <= 0 or out_w <= 0:
        raise ValueError("polygon_masks_u8: need at least one image and a positive output size")
    verts, offsets, classes, images, counts = _check_polygons("polygon_masks_u8", polys, sizes)
    p = len(classes)
    if p == 0:                               # nothing to draw: all background
        return torch.zeros((n, out_h, out_w), dtype=torch.uint8, device=device)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device, non_blocking=True)

    yi, xi = _nearest_tables(sizes, out_h, out_w, device)
    hw = dev(np.asarray(sizes, dtype=np.int32).reshape(n, 2))
    v_d, o_d, c_d, i_d = dev(verts), dev(offsets), dev(classes), dev(images)
    out = torch.empty((n, out_h, out_w), dtype=torch.uint8, device=device)
    L.check(L.lib().unet_polygon_mask_u8(_ptr(v_d), _ptr(o_d), _ptr(c_d), _ptr(i_d), p, int(counts.max()), _ptr(hw), n,
                                         out_h, out_w, _ptr(yi), _ptr(xi), _ptr(out), _stream()), "unet_polygon_mask_u8")
    return out


def polygon_class_histogram(polys, src_sizes, device="cuda") -> torch.Tensor:
    """Per-image histogram of raw-class bit sets (unet_polygon_class_histogram): int64 [N, 8], ``hist[i][b]`` = pixels of
    image ``i`` at its native size whose covering raw classes are exactly the bits of ``b`` (1 = raw 0 pitting, 2 = raw 1
    spalling, 4 = raw 2 scrape).  Everything ``analyze_class_overlaps.py`` of the reference reports per file (pixels per
    class, pairwise and triple overlaps, the classes after priority resolution) is a sum of these bins; no mask leaves
    the chip.  ``polys`` / ``src_sizes`` as for ``polygon_masks_u8``, coverage by the same rule; widths at most
    ``POLY_MAX_WIDTH``.  With no polygons the histogram is ``hist[i][0] = h * w``, without a launch."""
    sizes = [(int(h), int(w)) for h, w in src_sizes]
    n = len(sizes)
    if n == 0:
        raise ValueError("polygon_class_histogram: need at least one image")
    verts, offsets, classes, images, counts = _check_polygons("polygon_class_histogram", polys, sizes)
    wide = [i for i, (_, w) in enumerate(sizes) if w > POLY_MAX_WIDTH]
    if wide:
        raise ValueError(f"polygon_class_histogram: image {wide[0]} is {sizes[wide[0]][1]} pixels wide; the kernel takes "
                         f"at most {POLY_MAX_WIDTH}")
    if n > 65535:
        raise ValueError("polygon_class_histogram: at most 65535 images per call")
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    p = len(classes)
    if p == 0:                               # nothing drawn: every pixel has the empty class set
        hist = torch.zeros((n, 8), dtype=torch.int64)
        hist[:, 0] = torch.tensor([h * w for h, w in sizes], dtype=torch.int64)
        return hist.to(device)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device, non_blocking=True)

    hw = dev(np.asarray(sizes, dtype=np.int32).reshape(n, 2))
    v_d, o_d, c_d, i_d = dev(verts), dev(offsets), dev(classes), dev(images)
    hist = torch.empty((n, 8), dtype=torch.int64, device=device)
    L.check(L.lib().unet_polygon_class_histogram(_ptr(v_d), _ptr(o_d), _ptr(c_d), _ptr(i_d), p, int(counts.max()),
                                                 _ptr(hw), n, max(h for h, _ in sizes), max(w for _, w in sizes),
                                                 _ptr(hist), _stream()), "unet_polygon_class_histogram")
    return hist


# ------------------------------------------------------------------------------------------------ synthetic anomalies
SYNTH_DTYPE = np.dtype([("apply", "<i4"), ("seed", "<u4"), ("cells_y", "<i4"), ("cells_x", "<i4"), ("threshold", "<f4"),
                        ("beta", "<f4"), ("one_minus_beta", "<f4"), ("src", "<i4"), ("shift_y", "<i4"), ("shift_x", "<i4"),
                        ("perm", "<i4"), ("reserved", "<i4")])          # struct unet_synth_desc
SYNTH_MAX_CELLS_LOG2 = 6                 # lattices of 1, 2, .. 64 cells per axis
SYNTH_PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))     # descriptor field `perm`

_synth_tables = {}


def _synth_axis_tables(length: int, device):
    """Where the pixel centres of an axis of ``length`` pixels fall in lattices of 1, 2, .. 64 cells (csrc/synth.hip):
    cell [7, length] int32 and (t, fade(t)) [7, 2, length] fp32 in device memory, cached per (length, device).  Pixel p
    of L cells: cell (2pL + L) // (2 length), t = the remainder over 2 length rounded to fp32, fade in fp32 with every
    operation rounding once."""
    key = (length, device.index)
    hit = _synth_tables.get(key)
    if hit is None:
        p = np.arange(length, dtype=np.int64)
        cell = np.empty((SYNTH_MAX_CELLS_LOG2 + 1, length), dtype=np.int32)
        tf = np.empty((SYNTH_MAX_CELLS_LOG2 + 1, 2, length), dtype=np.float32)
        for lg in range(SYNTH_MAX_CELLS_LOG2 + 1):
            num = (2 * p + 1) << lg
            cell[lg] = num // (2 * length)
            t = ((num % (2 * length)).astype(np.float64) / np.float64(2 * length)).astype(np.float32)
            six, fifteen, ten = np.float32(6), np.float32(15), np.float32(10)
            tf[lg, 0] = t
            tf[lg, 1] = t * t * t * (t * (t * six - fifteen) + ten)
        hit = _synth_tables[key] = (torch.from_numpy(cell).to(device), torch.from_numpy(tf).to(device))
    return hit


def _synth_gradients(device):
    """The 256 unit gradient vectors (cos, sin)(2 pi k / 256), computed in double and rounded to fp32; uploaded once."""
    key = ("gradients", device.index)
    hit = _synth_tables.get(key)
    if hit is None:
        a = 2.0 * np.pi * np.arange(256, dtype=np.float64) / 256.0
        hit = _synth_tables[key] = torch.from_numpy(np.stack([np.cos(a), np.sin(a)], 1).astype(np.float32)).to(device)
    return hit


def synth_table(n: int, apply, seed, cells_y, cells_x, threshold, beta, src, shift_y, shift_x, perm) -> np.ndarray:
    """struct unet_synth_desc[n]; every argument is a scalar or a sequence of n.  ``one_minus_beta`` is set here, as the
    fp32 difference 1 - fp32(beta)."""
    rec = np.zeros(n, dtype=SYNTH_DTYPE)
    rec["apply"] = np.asarray(apply, dtype=bool)
    rec["seed"] = np.asarray(seed, dtype=np.int64) & 0xFFFFFFFF
    rec["cells_y"], rec["cells_x"], rec["threshold"] = cells_y, cells_x, threshold
    rec["beta"] = beta
    rec["one_minus_beta"] = np.float32(1) - rec["beta"]
    rec["src"], rec["shift_y"], rec["shift_x"], rec["perm"] = src, shift_y, shift_x, perm
    return rec


def synth_anomalies(images: torch.Tensor, desc: np.ndarray, masks: Optional[torch.Tensor] = None):
    """Corrupt a batch of normalised fp32 [N, 3, H, W] device images inside per-image Perlin masks (unet_synth_anomalies;
    the definition is at the top of csrc/synth.hip): where image i's noise exceeds its threshold the pixel becomes
    ``beta * x + one_minus_beta * donor``, the donor being image ``src`` of the batch, cyclically shifted and with its
    channels permuted.  ``desc`` = synth_table(...) of the batch size.  Returns (corrupted [N, 3, H, W], mask [N, 1, H, W]
    fp32) with mask = max(masks, m), m in {0, 1}; one launch, one small host-to-device copy, no synchronisation."""
    _require_cuda(images, masks)
    if images.dtype != torch.float32 or images.dim() != 4:
        raise ValueError("synth_anomalies expects a float32 [N, 3, H, W] device tensor")
    n, c, h, w = images.shape
    if not isinstance(desc, np.ndarray) or desc.dtype != SYNTH_DTYPE or desc.shape != (n,):
        raise ValueError("desc: expected synth_table(...) of the batch size")
    if masks is not None and (masks.dtype != torch.float32 or tuple(masks.shape) != (n, 1, h, w)):
        raise ValueError("masks: expected a float32 [N, 1, H, W] device tensor")
    images = images.contiguous()
    masks = None if masks is None else masks.contiguous()
    dev = images.device
    desc = np.ascontiguousarray(desc)
    corrupted = torch.empty_like(images)
    out_masks = torch.empty((n, 1, h, w), dtype=torch.float32, device=dev)
    if c == 3 and n > 0 and 0 < h < 32768 and 0 < w < 32768:
        (ycell, ytf), (xcell, xtf) = _synth_axis_tables(h, dev), _synth_axis_tables(w, dev)
    else:                                    # the library refuses such a batch before it reads any table
        ycell = ytf = xcell = xtf = out_masks
    desc_dev = torch.from_numpy(desc.view(np.uint8).reshape(n, -1)).to(dev, non_blocking=True)
    L.check(L.lib().unet_synth_anomalies(_ptr(images), _ptr(masks), n, c, h, w, _ptr(desc_dev),
                                         desc.ctypes.data_as(C.c_void_p), _ptr(ycell), _ptr(ytf), _ptr(xcell), _ptr(xtf),
                                         _ptr(_synth_gradients(dev)), _ptr(corrupted), _ptr(out_masks), _stream()),
            "unet_synth_anomalies")
    return corrupted, out_masks


class AnomalySynthesizer:
    """Synthetic anomalies for training on defect-free images (DRAEM / CutPaste style), on the GPU: with probability ``p``
    an image is corrupted inside a thresholded Perlin-noise mask by blending in another (or the same, shifted) image of
    its batch, and the mask becomes its segmentation truth.  ``corrupt(images, masks)`` -> (corrupted, masks) is what
    ``train_utils.train_epoch(..., corrupt=...)`` takes.

    ``draw(n, size)`` makes the per-sample parameters from this object's own generator (``size`` = the frames' (h, w):
    the shifts are drawn inside it); pass them back as ``params`` to replay a batch (tests do)."""

    def __init__(self, p=0.5, threshold=0.5, beta=(0.1, 0.8), max_cells_log2=SYNTH_MAX_CELLS_LOG2, seed: Optional[int] = None):
        if not 0.0 <= p <= 1.0:
            raise ValueError("p must lie in [0, 1]")
        if not 0 <= int(max_cells_log2) <= SYNTH_MAX_CELLS_LOG2:
            raise ValueError(f"max_cells_log2 must lie in 0..{SYNTH_MAX_CELLS_LOG2}")
        self.p, self.threshold = float(p), float(threshold)
        self.beta = (float(beta[0]), float(beta[1]))
        self.max_cells_log2 = int(max_cells_log2)
        self.gen = torch.Generator()
        if seed is not None:
            self.gen.manual_seed(int(seed))

    def draw(self, n: int, size) -> dict:
        h, w = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
        g = self.gen

        def ints(high, count=n):
            return torch.randint(0, high, (count,), generator=g).tolist()

        apply = (torch.rand(n, generator=g) < self.p).tolist()
        cells_y = [1 << k for k in ints(self.max_cells_log2 + 1)]
        cells_x = [1 << k for k in ints(self.max_cells_log2 + 1)]
        beta = torch.empty(n).uniform_(self.beta[0], self.beta[1], generator=g).tolist()
        src, shift_y, shift_x = ints(n), ints(h), ints(w)
        perm, seed = ints(6), ints(1 << 32)
        for i in range(n):
            if src[i] == i and shift_y[i] == 0 and shift_x[i] == 0:      # a donor equal to the image would change nothing
                if h * w == 1:
                    apply[i] = False
                else:
                    shift_y[i], shift_x[i] = divmod(1 + ints(h * w - 1, 1)[0], w)
        return {"apply": apply, "seed": seed, "cells_y": cells_y, "cells_x": cells_x, "beta": beta, "src": src,
                "shift_y": shift_y, "shift_x": shift_x, "perm": perm}

    def table(self, params: dict) -> np.ndarray:
        return synth_table(len(params["apply"]), threshold=self.threshold, **params)

    def __call__(self, images: torch.Tensor, masks: Optional[torch.Tensor] = None, params: Optional[dict] = None):
        if params is None:
            params = self.draw(images.shape[0], images.shape[-2:])
        return synth_anomalies(images, self.table(params), masks)
