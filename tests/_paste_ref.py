"""numpy int64 restatement of unet_paste_crop_u8 (include/unet_hip.h, csrc/paste.hip) and of crops.paste_matrix, built on
tests/_crops_ref.py: the yardstick of tests/test_cpu_paste.py and tests/test_gpu_paste.py, and the fixture both use.
Written from the rule, not from the kernel: whole crops at a time, no lanes, no store paths."""
import math

import numpy as np

import _crops_ref as R

ONE = 65536
PASTE_MAX = 8
SIZES = [(5, 7), (12, 9), (1, 1), (33, 40)]             # the ragged batch of tests/test_gpu_crops.py


def paste_matrix(donor_cx, donor_cy, scale, angle_deg, flip, tx, ty):
    """crop_matrix's formula with the crop centre replaced by the target point (tx, ty)"""
    f = -1.0 if flip else 1.0
    t = math.radians(float(angle_deg))
    b0, b1 = f * scale * math.cos(t), -scale * math.sin(t)
    b3, b4 = f * scale * math.sin(t), scale * math.cos(t)
    b2 = donor_cx + b0 * (0.5 - tx) + b1 * (0.5 - ty)
    b5 = donor_cy + b3 * (0.5 - tx) + b4 * (0.5 - ty)
    return [int(math.floor(v * 65536.0 + 0.5)) for v in (b0, b1, b2, b3, b4, b5)]


def _grid(out_h, out_w):
    return np.meshgrid(np.arange(out_h, dtype=np.int64), np.arange(out_w, dtype=np.int64), indexing="ij")


def bilinear(img, u, v):
    """the crop rule's bilinear value at (u, v), taps clamped into the image, WITHOUT its inside test: int64 [.., C]"""
    img = np.asarray(img).astype(np.int64)
    h, w = img.shape[:2]
    ub, vb = u - 32768, v - 32768
    x0, y0 = ub >> 16, vb >> 16
    fx, fy = ((ub & 0xFFFF) >> 8)[..., None], ((vb & 0xFFFF) >> 8)[..., None]
    x1, y1 = np.clip(x0 + 1, 0, w - 1), np.clip(y0 + 1, 0, h - 1)
    x0, y0 = np.clip(x0, 0, w - 1), np.clip(y0, 0, h - 1)
    top = (256 - fx) * img[y0, x0] + fx * img[y0, x1]
    bot = (256 - fx) * img[y1, x0] + fx * img[y1, x1]
    return ((256 - fy) * top + fy * bot + 32768) >> 16


def pack(arrays):
    """(bytes, offsets, sizes) of arrays packed one after another"""
    nbytes = [a.size for a in arrays]
    offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    return np.concatenate([np.asarray(a).reshape(-1) for a in arrays]), offsets, [a.shape[:2] for a in arrays]


def paste_crops(src, offsets, sizes, n_images, mask_src, mask_offsets, descs, paste_start, pastes, out_h, out_w, fill,
                ignore, src_bytes=None, mask_bytes=None, whole_dst=False):
    """(image crops uint8 [K, h, w, 3], mask crops uint8 [K, h, w], info) from the packed buffers and the tables the
    library takes: ``descs`` = [(image, a)], ``pastes`` = [(donor image, b, box, dst)] in table order, ``paste_start``
    [K + 1].  ``whole_dst``: look at every paste over the whole crop instead of its ``dst``.  ``info[k]`` lists, for every
    paste of crop k that was looked at, in order: ``alpha`` (the weight map, 0 where the paste does not act), and which
    pixels changed their ``label`` and their ``image`` bytes."""
    src_bytes = len(src) if src_bytes is None else src_bytes
    mask_bytes = len(mask_src) if mask_bytes is None else mask_bytes
    n_pastes = len(pastes)
    y, x = _grid(out_h, out_w)

    def image_of(i, buf, offs, c, nbytes):
        if not 0 <= i < n_images or not R.readable(offs[i], sizes[i], c, nbytes):
            return None
        h, w = (int(s) for s in sizes[i])
        return np.asarray(buf[int(offs[i]):int(offs[i]) + h * w * c]).reshape(h, w, c)

    out_i, out_m, info = [], [], []
    for k, (image, a) in enumerate(descs):
        img, msk = image_of(image, src, offsets, 3, src_bytes), image_of(image, mask_src, mask_offsets, 1, mask_bytes)
        pix = (R.crop(img, a, out_h, out_w, 1, fill) if img is not None
               else np.full((out_h, out_w, 3), fill, np.uint8)).astype(np.int64)
        lab = (R.crop(msk, a, out_h, out_w, 0, ignore)[..., 0] if msk is not None
               else np.full((out_h, out_w), ignore, np.uint8)).astype(np.int64)
        seen = []
        if n_pastes > 0 and img is not None and msk is not None:
            inside = R.inside_mask(sizes[image], a, out_h, out_w)
            first = int(paste_start[k])
            for i in range(min(int(paste_start[k + 1]) - first, PASTE_MAX)):
                donor, b, box, dst = pastes[min(max(first + i, 0), n_pastes - 1)]
                b = [int(t) for t in b]
                if whole_dst:
                    dst = (0, 0, out_w, out_h)
                sel = inside & (x >= dst[0]) & (x < dst[2]) & (y >= dst[1]) & (y < dst[3])
                dimg, dmsk = image_of(donor, src, offsets, 3, src_bytes), image_of(donor, mask_src, mask_offsets, 1, mask_bytes)
                alpha = np.zeros((out_h, out_w), np.int64)
                before = (lab.copy(), pix.copy())
                if dimg is not None and dmsk is not None:
                    dh, dw = dimg.shape[:2]
                    bx0, by0, bx1, by1 = max(int(box[0]), 0), max(int(box[1]), 0), min(int(box[2]), dw), min(int(box[3]), dh)
                    dm = dmsk[..., 0].astype(np.int64)

                    def member(px, py):
                        m = dm[np.clip(py, 0, dh - 1), np.clip(px, 0, dw - 1)]
                        return (px >= bx0) & (px < bx1) & (py >= by0) & (py < by1) & (m != 0) & (m != ignore)

                    u, v = b[0] * x + b[1] * y + b[2], b[3] * x + b[4] * y + b[5]
                    nx, ny = u >> 16, v >> 16
                    near = sel & member(nx, ny)
                    lab = np.where(near, dm[np.clip(ny, 0, dh - 1), np.clip(nx, 0, dw - 1)], lab)
                    ub, vb = u - 32768, v - 32768
                    tx, ty, fx, fy = ub >> 16, vb >> 16, (ub & 0xFFFF) >> 8, (vb & 0xFFFF) >> 8
                    alpha = (member(tx, ty) * (256 - fx) * (256 - fy) + member(tx + 1, ty) * fx * (256 - fy)
                             + member(tx, ty + 1) * (256 - fx) * fy + member(tx + 1, ty + 1) * fx * fy) * sel
                    assert alpha.min() >= 0 and alpha.max() <= 65536
                    d = bilinear(dimg, u, v)
                    mixed = (alpha[..., None] * d + (65536 - alpha[..., None]) * pix + 32768) >> 16
                    pix = np.where((alpha > 0)[..., None], mixed, pix)
                seen.append({"alpha": alpha, "label": lab != before[0], "image": (pix != before[1]).any(-1)})
        assert pix.min() >= 0 and pix.max() <= 255 and lab.min() >= 0 and lab.max() <= 255
        out_i.append(pix.astype(np.uint8))
        out_m.append(lab.astype(np.uint8))
        info.append(seen)
    return np.stack(out_i), np.stack(out_m), info


def tables(pastes, n_crops, dst_box):
    """([(donor, b, box, dst)] sorted stably by crop, paste_start) from [(crop, donor, b, box)]; ``dst_box(b, box)``
    makes a paste's dst"""
    order = sorted(range(len(pastes)), key=lambda j: pastes[j][0])
    counts = np.bincount([p[0] for p in pastes], minlength=n_crops) if pastes else np.zeros(n_crops, np.int64)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return [(pastes[j][1], pastes[j][2], pastes[j][3], dst_box(pastes[j][2], pastes[j][3])) for j in order], start


# ------------------------------------------------------------------------------------------------ the fixture
def shift(dy, dx):
    """centre to centre: output (y, x) <- source (y + dy, x + dx)"""
    return [ONE, 0, dx * ONE + ONE // 2, 0, ONE, dy * ONE + ONE // 2]


# the blobs of the fixture's masks: image -> [(class, (x0, y0, x1, y1))]
BLOBS = {0: [(1, (2, 1, 6, 4))], 1: [(2, (2, 3, 7, 9))], 2: [(3, (0, 0, 1, 1))],
         3: [(1, (5, 4, 15, 12)), (2, (18, 14, 30, 24)), (3, (32, 26, 40, 33)), (3, (0, 0, 6, 5))]}


def fixture(seed=0):
    """(images [h, w, 3], masks [h, w]) of SIZES: random bytes; random blobs of classes 1..3 inside BLOBS' boxes (three
    pixels in four set), image 3's second blob also holding a patch of 255 (the ignore value: no member) and one of 200
    (a member like any other label)"""
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
    masks = []
    for i, (h, w) in enumerate(SIZES):
        m = np.zeros((h, w), np.uint8)
        for cls, (x0, y0, x1, y1) in BLOBS[i]:
            m[y0:y1, x0:x1] = np.where(rng.random((y1 - y0, x1 - x0)) < 0.75, cls, 0)
        masks.append(m)
    masks[2][0, 0] = 3
    masks[3][17:20, 22:25] = 255
    masks[3][19:22, 25:28] = 200
    return images, masks


def cases(oh, ow):
    """(descs, pastes): nine crops of ``oh x ow`` and the pastes [(crop, donor, b, box)] of every kind; crop 8 carries
    nine, one more than counts, so only the library itself takes it (the wrapper takes descs[:8] and the pastes of
    crops 0..7)"""
    m = lambda *a: R.crop_matrix(*a, oh, ow)                            # noqa: E731
    tx, ty = ow / 2, oh / 2
    pm = lambda cx, cy, s, ang, f, x=tx, y=ty: paste_matrix(cx, cy, s, ang, f, x, y)       # noqa: E731
    box_a, box_b, box_c, box_d = (b for _, b in BLOBS[3])
    descs = [(3, shift(2, 3)), (3, shift(2, 3)), (3, m(20.0, 16.0, 1.0, 10.0, False)), (3, m(19.6, 16.2, 2.0, 5.0, False)),
             (1, shift(-2, 0)), (0, shift(0, 0)), (1, shift(0, 0)), (3, shift(33 - oh, 40 - ow)), (3, shift(2, 3))]
    # blob B's middle (24, 19) on the crop's middle, centre to centre (ow, oh may be odd: whole-pixel shifts)
    c2c = shift(19 - oh // 2, 24 - ow // 2)
    flipped = [-ONE, 0, (24 + (ow - 1) // 2) * ONE + ONE // 2, 0, ONE, (19 - oh // 2) * ONE + ONE // 2]
    pastes = [
        (0, 3, c2c, box_b),                                             # centre to centre; the donor is the base image
        (1, 3, flipped, box_b),                                         # the same paste, flipped
        (2, 3, pm(10.0, 8.0, 1.0, 37.0, False), box_a), (2, 3, pm(24.0, 19.0, 1.0, 90.0, True), box_b),    # overlapping
        (3, 3, pm(24.0, 19.0, 0.5, 0.0, False, ow / 4, oh / 4), box_b),
        (3, 1, pm(4.5, 6.0, 2.0, -20.0, False, 3 * ow / 4, oh / 2), BLOBS[1][0][1]),
        (3, 3, pm(10.0, 8.0, 4.0, 15.0, True, ow / 2, 3 * oh / 4), box_a),
        (4, 3, pm(10.0, 8.0, 1.0, 0.0, False, ow / 2, 2.0), box_a),     # onto the crop that hangs off its image's top
        (5, 2, pm(0.5, 0.5, 0.4, 30.0, False, 1.5, 1.5), (0, 0, 1, 1)),                 # the 1 x 1 image as donor
        (5, 3, pm(36.0, 30.0, 1.5, 12.0, False, 4.0, 2.5), box_c),            # a box on the image's edge
        (5, 3, pm(2.0, 2.0, 0.7, -8.0, False, 2.5, 2.0), (-5, -3, 8, 6)),          # boxes crossing it
        (5, 1, pm(4.5, 6.0, 1.0, 0.0, True, 1.5, 3.0), (1, 2, 12, 14)),
    ]
    # exactly eight on crop 6, nine on crop 8: alternating donors and classes, walking across the crop
    many = [(3, (10.0, 8.0), box_a), (3, (24.0, 19.0), box_b), (0, (4.0, 2.5), BLOBS[0][0][1]), (3, (36.0, 29.5), box_c),
            (1, (4.5, 6.0), BLOBS[1][0][1]), (3, (3.0, 2.5), box_d), (2, (0.5, 0.5), (0, 0, 1, 1)), (3, (24.0, 19.0), box_b),
            (3, (10.0, 8.0), box_a)]
    for crop, n in ((6, 8), (8, 9)):
        for j in range(n):
            donor, (cx, cy), box = many[j]
            pastes.append((crop, donor, pm(cx, cy, 0.6 + 0.2 * (j % 3), 40.0 * j, bool(j % 2),
                                           (j % 4 + 0.5) * ow / 4, (j % 3 + 0.5) * oh / 3), box))
    return descs, pastes
