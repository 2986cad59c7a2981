"""numpy restatement of the visualisation sheet (csrc/render.hip, ops.render_sheet): the two colour tables, the five
panel kinds and the sheet assembly, byte for byte.  tests/test_cpu_render.py pins every piece of it to matplotlib's own
arithmetic; tests/test_gpu_render.py holds the device to it.  matplotlib is not imported here."""
import numpy as np

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
WHITE = np.array([255, 255, 255], np.uint8)

# matplotlib's `hot`: per channel the (x, y) knots of a piecewise-linear map, clamped outside
HOT_KNOTS = (((0.0, 0.0416), (0.365079, 1.0), (1.0, 1.0)),
             ((0.0, 0.0), (0.365079, 0.0), (0.746032, 1.0), (1.0, 1.0)),
             ((0.0, 0.0), (0.746032, 0.0), (1.0, 1.0)))


def _piecewise(knots, x):
    for (x0, y0), (x1, y1) in zip(knots, knots[1:]):
        if x <= x1:
            return ((x - x0) / (x1 - x0)) * (y1 - y0) + y0
    return knots[-1][1]


def lut(name):
    """(256, 3) uint8: floor(255 * L(x_k)) in float64 at x_k = k * (1 / 255), x_255 = 1: the product, as numpy's linspace
    forms it, lies below k / 255 for some k, and 255 * x_k then falls below k."""
    out = np.zeros((256, 3), np.uint8)
    step = np.float64(1.0) / np.float64(255.0)
    for k in range(256):
        x = np.float64(k) * step if k < 255 else np.float64(1.0)
        for c in range(3):
            v = x if name == "gray" else _piecewise(HOT_KNOTS[c], x)
            out[k, c] = int(np.floor(np.float64(255.0) * min(max(v, 0.0), 1.0)))
    return out


LUTS = {"gray": lut("gray"), "hot": lut("hot")}


def plane_range(x):
    """(lo, hi) over the finite pixels of one plane as float32, or None when there is none."""
    x = np.asarray(x, np.float32)
    fin = x[np.isfinite(x)]
    return (fin.min(), fin.max()) if fin.size else None


def panel_range(t):
    """(N, 2) float32 of [N, ...] planes; NaN for a plane without a finite pixel."""
    t = np.asarray(t, np.float32)
    out = np.full((t.shape[0], 2), np.nan, np.float32)
    for n in range(t.shape[0]):
        r = plane_range(t[n])
        if r is not None:
            out[n] = r
    return out


def map_index(x, index_dtype=np.float64, clip_hi=255, finite_range=True):
    """(index (H, W) int, drawn (H, W) bool) of one plane.  The keyword arguments plant defects (tests only)."""
    x = np.asarray(x, np.float32)
    fin = np.isfinite(x)
    idx = np.zeros(x.shape, np.int64)
    if not fin.any():
        return idx, fin
    pool = x[fin] if finite_range else x[~np.isnan(x)]
    lo, hi = index_dtype(pool.min()), index_dtype(pool.max())
    if hi > lo:
        with np.errstate(invalid="ignore", over="ignore"):
            t = (x.astype(index_dtype) - lo) / (hi - lo)
            s = np.floor(t * index_dtype(256.0))
        s = np.where(fin & ~np.isnan(s), s, 0.0)           # (NaN only under a planted range defect)
        idx = np.clip(s, 0, clip_hi).astype(np.int64)
    return idx, fin


def map_panel(x, name, **defect):
    """(H, W, 3) uint8 of a gray / hot panel."""
    idx, drawn = map_index(x, **defect)
    table = np.concatenate([LUTS[name], np.zeros((1, 3), np.uint8)])       # entry 256: what a planted clip defect reads
    return np.where(drawn[..., None], table[idx], WHITE)


def unit_bytes(v, rounding=False):
    """clamp to [0, 1] (NaN -> 0), byte = trunc(v * 255) in float32."""
    v = np.asarray(v, np.float32)
    v = np.where(v > 0, v, np.float32(0))
    v = np.where(v > 1, np.float32(1), v).astype(np.float32)
    p = v * np.float32(255.0)
    return (np.rint(p) if rounding else p).astype(np.uint8)


def unit_panel(x, **defect):
    """(3, H, W) float32 in [0, 1] -> (H, W, 3) uint8."""
    return unit_bytes(np.asarray(x, np.float32).transpose(1, 2, 0), **defect)


def image_panel(x, mean=MEAN, std=STD, **defect):
    """(3, H, W) float32, normalised -> (H, W, 3) uint8: x * std rounded, + mean rounded, both float32."""
    x = np.asarray(x, np.float32)
    s = np.asarray(std, np.float32).reshape(3, 1, 1)
    m = np.asarray(mean, np.float32).reshape(3, 1, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (x * s).astype(np.float32) + m
    return unit_panel(v, **defect)


def alpha8(alpha):
    return int(round(255 * float(alpha)))


def overlay_panel(image, amap, alpha, mean=MEAN, std=STD):
    img = image_panel(image, mean, std).astype(np.int64)
    idx, drawn = map_index(amap)
    heat = LUTS["hot"][idx].astype(np.int64)
    a8 = alpha8(alpha)
    mixed = (a8 * heat + (255 - a8) * img + 127) // 255
    return np.where(drawn[..., None], mixed, img).astype(np.uint8)


def _plane(t):
    t = np.asarray(t, np.float32)
    return t[0] if t.ndim == 3 else t


def panel(col, n, mean=MEAN, std=STD):
    kind = col[0]
    if kind == "image":
        return image_panel(col[1][n], mean, std)
    if kind == "unit":
        return unit_panel(col[1][n])
    if kind in ("gray", "hot"):
        return map_panel(_plane(col[1][n]), kind)
    if kind == "overlay":
        return overlay_panel(col[1][n], _plane(col[2][n]), col[3], mean, std)
    raise ValueError(kind)


def assemble(panels, gutter_y, gutter_x):
    """panels[n][k]: (H, W, 3) uint8 -> the sheet (N H + (N - 1) gy, K W + (K - 1) gx, 3), gutters 255.  (The product
    has one gutter for both axes; two here, so that a test can exchange them.)"""
    n, k = len(panels), len(panels[0])
    h, w = panels[0][0].shape[:2]
    sheet = np.full((n * h + (n - 1) * gutter_y, k * w + (k - 1) * gutter_x, 3), 255, np.uint8)
    for i in range(n):
        for j in range(k):
            y, x = i * (h + gutter_y), j * (w + gutter_x)
            sheet[y:y + h, x:x + w] = panels[i][j]
    return sheet


def render_sheet(columns, gutter=4, mean=MEAN, std=STD):
    """columns as ops.render_sheet takes them, with numpy arrays: the sheet as (rows, cols, 3) uint8."""
    columns = [tuple(np.asarray(v, np.float32) if i in (1, 2) and not np.isscalar(v) else v for i, v in enumerate(c))
               for c in columns]
    n = columns[0][1].shape[0]
    return assemble([[panel(c, i, mean, std) for c in columns] for i in range(n)], gutter, gutter)
