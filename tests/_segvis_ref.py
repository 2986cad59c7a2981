"""numpy restatement of the segmentation prediction sheets (csrc/segvis.hip, ops.seg_confidence, ops.class_palette,
ops.viridis_lut, ops.render_seg_sheet): the two palette modes, the viridis index, the four panel kinds, the per_row
assembly, and float64 labels and confidence.  tests/test_cpu_segvis.py pins the tables and the index rule to matplotlib;
tests/test_gpu_segvis.py holds the device to this file.  matplotlib is not imported here: the viridis bytes are read
from the table the product embeds, which the CPU test compares with matplotlib entry by entry."""
import numpy as np

import _render_ref as R

WHITE = R.WHITE
TAB10 = np.array([[31, 119, 180], [255, 127, 14], [44, 160, 44], [214, 39, 40], [148, 103, 189], [140, 86, 75],
                  [227, 119, 194], [127, 127, 127], [188, 189, 34], [23, 190, 207]], np.uint8)
SCALED_ENTRIES = {2: [0, 9], 3: [0, 5, 9], 4: [0, 3, 6, 9], 8: [0, 1, 2, 4, 5, 7, 8, 9]}      # the issue's list


def tab10_entry(i, num_classes, mode):
    """index: cmap(i).  scaled: imshow(vmin=0, vmax=C-1) -> Normalize, then the colour map's floor(x * N), x == 1 -> N - 1."""
    if mode == "index":
        return i
    x = np.float64(i) / np.float64(num_classes - 1)
    return min(int(np.floor(x * np.float64(10.0))), 9)


def class_palette(num_classes, mode):
    out = np.full((256, 3), 255, np.uint8)
    for i in range(num_classes):
        out[i] = TAB10[tab10_entry(i, num_classes, mode)]
    return out


def viridis_lut():
    from tiaozhanbei_unet_amd._viridis import VIRIDIS
    return np.frombuffer(VIRIDIS, np.uint8).reshape(256, 3).copy()


def lut_index(v):
    """(index, drawn) of a float32 map over the fixed range [0, 1]: floor(v * 256) clipped to [0, 255]; v < 0 -> 0;
    non-finite pixels are not drawn."""
    v = np.asarray(v, np.float32)
    fin = np.isfinite(v)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.floor(np.where(fin, v, np.float32(0)).astype(np.float64) * 256.0)
    return np.clip(s, 0, 255).astype(np.int64), fin


def lut_panel(v, lut):
    idx, drawn = lut_index(v)
    return np.where(drawn[..., None], np.asarray(lut, np.uint8)[idx], WHITE)


def label_bytes(labels):
    """what ops.render_seg_sheet makes of an integer mask: values outside 0..255 become 255"""
    a = np.asarray(labels)
    if a.dtype == np.uint8:
        return a
    a = a.astype(np.int64)
    return np.where((a < 0) | (a > 255), 255, a).astype(np.uint8)


def classes_panel(labels, palette):
    return np.asarray(palette, np.uint8)[label_bytes(labels).astype(np.int64)]


def overlay_panel(image, labels, alpha, palette):
    img = R.image_panel(image).astype(np.int64)
    lab = label_bytes(labels).astype(np.int64)
    top = np.asarray(palette, np.uint8)[lab].astype(np.int64)
    a8 = R.alpha8(alpha)
    mixed = (a8 * top + (255 - a8) * img + 127) // 255
    return np.where((lab == 0)[..., None], img, mixed).astype(np.uint8)


def panel(col, image, i, palette, lut):
    kind = col[0]
    if kind == "image":
        return R.image_panel(image[i])
    if kind == "classes":
        return classes_panel(col[1][i], palette)
    if kind == "overlay":
        return overlay_panel(image[i], col[1][i], col[2], palette)
    if kind == "lut":
        return lut_panel(col[1][i], lut)
    raise ValueError(kind)


def sheet_shape(n, k, h, w, gutter, per_row):
    rows = -(-n // per_row)
    return rows * h + (rows - 1) * gutter, per_row * k * w + (per_row * k - 1) * gutter, 3


def assemble(panels, h, w, gutter, per_row):
    """panels[i][j]: (h, w, 3) uint8 of sample i, panel j -> the sheet; gutters and the cells past n are 255."""
    n, k = len(panels), len(panels[0])
    sheet = np.full(sheet_shape(n, k, h, w, gutter, per_row), 255, np.uint8)
    for i in range(n):
        r, cell = divmod(i, per_row)
        for j in range(k):
            y, x = r * (h + gutter), (cell * k + j) * (w + gutter)
            sheet[y:y + h, x:x + w] = panels[i][j]
    return sheet


def render_seg_sheet(images, columns, gutter=4, per_row=1, palette=None, lut=None):
    """images and columns as ops.render_seg_sheet takes them, with numpy arrays."""
    images = np.asarray(images, np.float32)
    palette = class_palette(10, "index") if palette is None else np.asarray(palette, np.uint8)
    lut = viridis_lut() if lut is None else np.asarray(lut, np.uint8)
    n, _, h, w = images.shape
    return assemble([[panel(c, images, i, palette, lut) for c in columns] for i in range(n)], h, w, gutter, per_row)


# ---- labels and confidence in float64 ---------------------------------------------------------------------------------
def labels64(logits, last_wins=False):
    """argmax over axis 1 of (N, C, ...) logits, the first maximum winning ties (last_wins plants the other rule)"""
    z = np.asarray(logits, np.float64)
    if last_wins:
        return (z.shape[1] - 1 - np.argmax(z[:, ::-1], axis=1)).astype(np.uint8)
    return np.argmax(z, axis=1).astype(np.uint8)


def conf64(logits):
    """softmax(z).max over classes = 1 / sum_j exp(z_j - max z), in float64"""
    z = np.asarray(logits, np.float64)
    return 1.0 / np.exp(z - z.max(axis=1, keepdims=True)).sum(axis=1)


def conf32(logits, subtract_max=True):
    """the kernel's formula in float32 on the host, class by class in order: what the measured expf term is taken from.
    subtract_max=False plants the defect of the formula without its max subtraction, 1 / sum_j expf(z_j)."""
    z = np.asarray(logits, np.float32)
    best = z.max(axis=1) if subtract_max else np.zeros(z[:, 0].shape, np.float32)
    s = np.zeros(best.shape, np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for j in range(z.shape[1]):
            s = (s + np.exp((z[:, j] - best).astype(np.float32)).astype(np.float32)).astype(np.float32)
        return (np.float32(1.0) / s).astype(np.float32)


def conf_bound(num_classes, host_rel):
    """Allowed relative error of conf, term by term (conf = 1 / s, s = sum_j e_j, e_j = expf(d_j), d_j = z_j - max z <= 0,
    s >= 1 as the maximum's own term is exactly 1; u = 2^-24 is one fp32 rounding):
      subtraction  d_j carries a relative rounding u, an absolute u |d_j|, which exp turns into a relative error u |d_j| of
                   e_j, an absolute u |d_j| e^{d_j} <= u / e (the maximum of x e^-x); summed over C terms and divided by
                   s >= 1: <= C e^-1 u
      additions    C - 1 fp32 additions of positive terms: <= (C - 1) u of s
      division     one correctly rounded division: u
      expf         measured: 4 x the worst relative error of the same fp32 formula on the host (host_rel), never less
                   than 2^-22 (the rule of _ref64.assert_measured for device math functions)
    -> (total, {term: value})"""
    u = 2.0 ** -24
    terms = {"subtraction": num_classes * np.exp(-1.0) * u, "additions": (num_classes - 1) * u, "division": u,
             "expf": max(4.0 * host_rel, 2.0 ** -22)}
    return sum(terms.values()), terms
