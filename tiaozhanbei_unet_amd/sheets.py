"""Sheets rendered on the device, outside autograd: the MVTec visualisation sheet and the segmentation prediction sheets."""
import ctypes as C

import torch

from . import _lib as L
from ._hipcall import _ptr, _require_cuda, _stream


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


def inverse_temperature(temperature, what="temperature"):
    """float32(1 / T) as a Python float, the ``inv_t`` of unet_seg_confidence_scaled and unet_temperature_sweep: the
    quotient in float64, rounded once.  ValueError unless both T and the rounded quotient are finite and > 0."""
    import math
    import struct
    t = float(temperature)
    if not (math.isfinite(t) and t > 0.0):
        raise ValueError(f"{what} {temperature!r} is not a finite value > 0")
    try:
        inv = struct.unpack("f", struct.pack("f", 1.0 / t))[0]
    except OverflowError:
        inv = math.inf
    if not (math.isfinite(inv) and inv > 0.0):
        raise ValueError(f"{what} {temperature!r}: 1 / T is not a finite float32 > 0")
    return inv


def seg_confidence(logits, labels=True, conf=True, temperature=1.0):
    """(labels, conf) of (N, C, H, W) logits, 2 <= C <= 8, as DEVICE tensors: labels uint8 (N, H, W) = the argmax (the
    first maximum wins ties, as torch.argmax), conf float32 (N, H, W) = softmax(logits, 1).max(1) computed in fp32 as
    1 / sum_j expf(z_j - max z) (reference visualize.py:134-135, visualize_kolektorsdd.py:131).  Either is None
    when not asked for.  ``temperature`` T != 1: the confidence of softmax(logits / T), 1 / sum_j expf((z_j - max z) *
    float32(1 / T)), with the labels still those of the raw logits (unet_seg_confidence_scaled).  One launch
    (unet_seg_confidence at T == 1); does not synchronise."""
    _require_cuda(logits)
    if logits.dim() != 4:
        raise ValueError(f"seg_confidence: logits are (N, C, H, W), got {tuple(logits.shape)}")
    if not (labels or conf):
        raise ValueError("seg_confidence: neither labels nor conf asked for")
    inv_t = 1.0 if float(temperature) == 1.0 else inverse_temperature(temperature, "seg_confidence: temperature")
    n, c, h, w = logits.shape
    x = logits.detach().float().contiguous()
    lab = torch.empty((n, h, w), dtype=torch.uint8, device=x.device) if labels else None
    cf = torch.empty((n, h, w), dtype=torch.float32, device=x.device) if conf else None
    if float(temperature) == 1.0:
        L.check(L.lib().unet_seg_confidence(_ptr(x), n, c, h * w, _ptr(lab), _ptr(cf), _stream()), "unet_seg_confidence")
    else:
        L.check(L.lib().unet_seg_confidence_scaled(_ptr(x), n, c, h * w, inv_t, _ptr(lab), _ptr(cf), _stream()),
                "unet_seg_confidence_scaled")
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
