"""numpy restatement of the tiled prediction (tiaozhanbei_unet_amd/tiling.py, csrc/tiles.hip): where the tiles go, and
the blend of their logits in float32 with the operation order the header states -- a loop over the covering tiles in
ascending i, then ascending j; integer weights summed in int32; product and sum rounded separately; one conversion and one
division; a pixel under exactly one tile copied.  Labels are the first-maximum argmax of the blended logits, the
confidence goes through _segvis_ref.conf32 / conf64.  tests/test_cpu_tiles.py pins this file by hand cases,
tests/test_gpu_tiles.py holds the device to it."""
import numpy as np

import _segvis_ref as S

MAX_TILES_AXIS = 64
MAX_RAMP = 256


def plan_axis(frame, tile, min_overlap):
    length = min(tile, frame)
    if not 0 <= min_overlap < length:
        raise ValueError((frame, tile, min_overlap))
    if frame <= tile:
        return [0]
    n = 1
    while length + (n - 1) * (length - min_overlap) < frame:      # n tiles reach at most this far
        n += 1
    if n > MAX_TILES_AXIS:
        raise ValueError((frame, tile, min_overlap, n))
    return [(i * (frame - length)) // (n - 1) for i in range(n)]


def default_ramp(origins, length):
    if len(origins) < 2:
        return 1
    return int(np.clip(min(a + length - b for a, b in zip(origins, origins[1:])), 1, MAX_RAMP))


def weights(length, ramp):
    """q(k) = min(k + 1, L - k, B) for k = 0 .. L - 1, int64"""
    k = np.arange(length, dtype=np.int64)
    return np.minimum(np.minimum(k + 1, length - k), ramp)


def gather(frame, th, tw, oy, ox):
    """tiles [len(oy) * len(ox), C, th, tw] of a frame [C, H, W]"""
    return np.stack([frame[:, y:y + th, x:x + tw] for y in oy for x in ox])


def blend(tiles, oy, ox, frame_hw, ramp_y, ramp_x):
    """(blended fp32 [C, H, W], wsum int64 [H, W], covers int64 [H, W]) of fp32 tile logits [T, C, th, tw]"""
    tiles = np.asarray(tiles, np.float32)
    _, c, th, tw = tiles.shape
    h, w = frame_hw
    qy, qx = weights(th, ramp_y), weights(tw, ramp_x)
    acc = np.zeros((c, h, w), np.float32)
    one = np.zeros((c, h, w), np.float32)
    wsum = np.zeros((h, w), np.int64)
    covers = np.zeros((h, w), np.int64)
    for i, y in enumerate(oy):
        for j, x in enumerate(ox):
            q = qy[:, None] * qx[None, :]                          # exact integers
            z = tiles[i * len(ox) + j]
            win = (slice(None), slice(y, y + th), slice(x, x + tw))
            first = covers[win[1:]] == 0
            one[win] = np.where(first[None], z, one[win])
            prod = (q.astype(np.float32)[None] * z).astype(np.float32)         # one rounding
            acc[win] = (acc[win] + prod).astype(np.float32)                    # one rounding
            wsum[win[1:]] += q
            covers[win[1:]] += 1
    assert covers.min() >= 1 and wsum.max() < 2 ** 31
    with np.errstate(over="ignore", invalid="ignore"):
        mixed = (acc / wsum.astype(np.float32)[None]).astype(np.float32)       # one conversion, one division
    return np.where((covers == 1)[None], one, mixed), wsum, covers


def labels_of(blended):
    """uint8 [H, W]: the first maximum over the classes of fp32 [C, H, W]"""
    return S.labels64(np.asarray(blended)[None])[0]


def predict(tiles, oy, ox, frame_hw, ramp_y, ramp_x):
    """(labels uint8, conf fp32 by the kernel's formula on the host, blended fp32)"""
    mixed, _, _ = blend(tiles, oy, ox, frame_hw, ramp_y, ramp_x)
    return labels_of(mixed), S.conf32(mixed[None])[0], mixed
