"""numpy int64 restatement of unet_affine_crop_u8 (include/unet_hip.h, csrc/crops.hip) and of crops.crop_matrix: the
yardstick of tests/test_cpu_crops.py and tests/test_gpu_crops.py.  Written from the rule, not from the kernel: whole
crops at a time, no lanes, no store paths."""
import math

import numpy as np


def crop_matrix(cx, cy, scale, angle_deg, flip, out_h, out_w):
    """source = (cx, cy) + scale R(angle) diag(-1 if flip else 1, 1) ((x + .5, y + .5) - (out_w / 2, out_h / 2)), each
    entry fixed as floor(v * 65536 + 0.5)"""
    f = -1.0 if flip else 1.0
    t = math.radians(float(angle_deg))
    a0, a1 = f * scale * math.cos(t), -scale * math.sin(t)
    a3, a4 = f * scale * math.sin(t), scale * math.cos(t)
    a2 = cx + a0 * (0.5 - out_w / 2) + a1 * (0.5 - out_h / 2)
    a5 = cy + a3 * (0.5 - out_w / 2) + a4 * (0.5 - out_h / 2)
    return [int(math.floor(v * 65536.0 + 0.5)) for v in (a0, a1, a2, a3, a4, a5)]


def crop(image, a, out_h, out_w, mode, fill):
    """One crop [out_h, out_w, C] of a uint8 image [H, W, C]."""
    img = np.asarray(image).astype(np.int64)
    h, w, c = img.shape
    a = [int(v) for v in a]
    y, x = np.meshgrid(np.arange(out_h, dtype=np.int64), np.arange(out_w, dtype=np.int64), indexing="ij")
    u = a[0] * x + a[1] * y + a[2]
    v = a[3] * x + a[4] * y + a[5]
    nx, ny = u >> 16, v >> 16
    inside = (nx >= 0) & (nx < w) & (ny >= 0) & (ny < h)
    if mode == 0:
        val = img[np.clip(ny, 0, h - 1), np.clip(nx, 0, w - 1)]
    else:
        ub, vb = u - 32768, v - 32768
        x0, y0 = ub >> 16, vb >> 16
        fx, fy = ((ub & 0xFFFF) >> 8)[..., None], ((vb & 0xFFFF) >> 8)[..., None]
        x1, y1 = np.clip(x0 + 1, 0, w - 1), np.clip(y0 + 1, 0, h - 1)
        x0, y0 = np.clip(x0, 0, w - 1), np.clip(y0, 0, h - 1)
        top = (256 - fx) * img[y0, x0] + fx * img[y0, x1]
        bot = (256 - fx) * img[y1, x0] + fx * img[y1, x1]
        val = ((256 - fy) * top + fy * bot + 32768) >> 16
    out = np.where(inside[..., None], val, fill)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def inside_mask(hw, a, out_h, out_w):
    """where output pixels fall inside an image of ``hw``"""
    y, x = np.meshgrid(np.arange(out_h, dtype=np.int64), np.arange(out_w, dtype=np.int64), indexing="ij")
    nx = (int(a[0]) * x + int(a[1]) * y + int(a[2])) >> 16
    ny = (int(a[3]) * x + int(a[4]) * y + int(a[5])) >> 16
    return (nx >= 0) & (nx < hw[1]) & (ny >= 0) & (ny < hw[0])


def readable(offset, hw, c, src_bytes):
    """the kernel's guard: does image [h][w][c] at ``offset`` lie inside src[0, src_bytes)?"""
    h, w = int(hw[0]), int(hw[1])
    return not (int(offset) < 0 or h <= 0 or w <= 0 or int(offset) + h * w * c > int(src_bytes))


def crops(images, descs, out_h, out_w, mode, fill, c=None, offsets=None, src=None):
    """[K, out_h, out_w, C]: ``descs`` = [(image index, a)].  With ``src`` (the packed bytes), ``offsets`` and sizes
    ``images`` = [(h, w)], the images are read out of the buffer and the guards apply (an index outside the list or an
    image outside the buffer: all fill); otherwise ``images`` are the arrays."""
    out = []
    for image, a in descs:
        if src is not None:
            ok = 0 <= image < len(images) and readable(offsets[image], images[image], c, len(src))
            img = None
            if ok:
                h, w = images[image]
                img = np.asarray(src[offsets[image]:offsets[image] + h * w * c]).reshape(h, w, c)
        else:
            ok = 0 <= image < len(images)
            img = images[image] if ok else None
            c = c or (np.asarray(images[0]).shape[2])
        out.append(crop(img, a, out_h, out_w, mode, fill) if ok else np.full((out_h, out_w, c), fill, np.uint8))
    return np.stack(out)
