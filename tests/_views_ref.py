"""numpy restatement of the view merge (tiaozhanbei_unet_amd/views.py, csrc/views.hip), operation for operation as the
header states it: the tap table of one axis in Python integers; the value of a view at a pixel in np.float32, every
product and every sum rounded once; a view of the frame's own size copied; the sum over the views in ascending order from
the first view's value, one division by (float)V; labels the first maximum of the merged logits; agreement the number of
views whose own first maximum is the merged label.  The confidence goes through _segvis_ref.conf32 / conf64.
tests/test_cpu_views.py pins this file by exact rational arithmetic and hand cases, tests/test_gpu_views.py holds the
device to it."""
import numpy as np

import _segvis_ref as S

MAX_VIEWS = 16
MAX_SIDE = 16384
FLIP_SETS = {"none": [(0, 0)], "h": [(0, 0), (1, 0)], "v": [(0, 0), (0, 1)], "all": [(0, 0), (1, 0), (0, 1), (1, 1)]}


def raw_tap(i, n_out, m_view):
    """p before the clamp: floor(((2 i + 1) M 2^15) / N) - 2^15, in Python integers"""
    return ((2 * i + 1) * m_view * 32768) // n_out - 32768


def taps(n_out, m_view, flip=False):
    """(i0, i1, f) int64 arrays over the N outputs of an axis with M view samples; a flipped axis reads the mirrored
    samples M - 1 - i0 and M - 1 - i1"""
    i0, i1, f = (np.zeros(n_out, np.int64) for _ in range(3))
    for i in range(n_out):
        if m_view == n_out:
            p = i << 16                                 # the tap i, fraction 0
        else:
            p = min(max(raw_tap(i, n_out, m_view), 0), (m_view - 1) << 16)
        i0[i], f[i] = p >> 16, p & 0xFFFF
        i1[i] = min(i0[i] + 1, m_view - 1)
    if flip:
        i0, i1 = m_view - 1 - i0, m_view - 1 - i1
    return i0, i1, f


def _lerp(f, a, b):
    """((float)(65536 - f) a + (float)f b) 2^-16, three roundings"""
    wa, wb = (65536 - f).astype(np.float32), f.astype(np.float32)
    pa = (wa * a).astype(np.float32)
    pb = (wb * b).astype(np.float32)
    return ((pa + pb).astype(np.float32) * np.float32(2.0 ** -16)).astype(np.float32)


def view_value(z, frame_hw, flip_x=False, flip_y=False):
    """fp32 [C, H, W]: the view's logits z [C, hv, wv] at the frame's pixels"""
    z = np.asarray(z, np.float32)
    _, hv, wv = z.shape
    h, w = frame_hw
    y0, y1, fy = taps(h, hv, flip_y)
    x0, x1, fx = taps(w, wv, flip_x)
    if (hv, wv) == (h, w):                              # not interpolated: the bits themselves
        return z[:, y0][:, :, x0].copy()
    fxb, fyb = fx[None, None, :], fy[None, :, None]
    with np.errstate(over="ignore", invalid="ignore"):
        top = _lerp(fxb, z[:, y0][:, :, x0], z[:, y0][:, :, x1])
        bot = _lerp(fxb, z[:, y1][:, :, x0], z[:, y1][:, :, x1])
        return _lerp(fyb, top, bot)


def first_max(z):
    """uint8 [H, W]: the first maximum over the classes of fp32 [C, H, W]"""
    return S.labels64(np.asarray(z)[None])[0]


def merge(view_logits, flips, frame_hw):
    """(merged fp32 [C, H, W], labels uint8 [H, W], agreement uint8 [H, W]) of the views' fp32 logits [C, hv, wv] and
    their (flip_x, flip_y)"""
    assert 1 <= len(view_logits) == len(flips) <= MAX_VIEWS
    acc, votes = None, []
    for z, (fx, fy) in zip(view_logits, flips):
        val = view_value(z, frame_hw, bool(fx), bool(fy))
        votes.append(first_max(val))
        with np.errstate(over="ignore", invalid="ignore"):
            acc = val if acc is None else (acc + val).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        merged = (acc / np.float32(len(view_logits))).astype(np.float32)
    labels = first_max(merged)
    agreement = np.sum([v == labels for v in votes], axis=0).astype(np.uint8)
    return merged, labels, agreement


def predict(view_logits, flips, frame_hw):
    """(labels uint8, conf fp32 by the kernel's formula on the host, agreement uint8, merged fp32)"""
    merged, labels, agreement = merge(view_logits, flips, frame_hw)
    return labels, S.conf32(merged[None])[0], agreement, merged


def plan_views(scales, flips):
    out = []
    for s in scales:
        if not 0.5 <= s <= 2.0:
            raise ValueError(s)
        for fx, fy in FLIP_SETS[flips]:
            if (float(s), fx, fy) not in out:
                out.append((float(s), fx, fy))
    if not 1 <= len(out) <= MAX_VIEWS:
        raise ValueError(len(out))
    return out
