"""Independent numpy restatement of the synthetic-anomaly definition (csrc/synth.hip): its own axis tables, gradient
table, hash, noise and blend.  ``noise32`` / ``synthesize`` use IEEE single precision with every product and sum rounded
once and in the kernel's order, so the kernel must equal them bit for bit; ``noise64`` is the same formula in float64
(only the gradient table and the fractions keep their fp32-rounded values: they are inputs of the formula), which
bounds what the fp32 arithmetic costs."""
import numpy as np

PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
_M32 = np.uint64(0xFFFFFFFF)


def gradients():
    k = np.arange(256, dtype=np.float64)
    return np.cos(2.0 * np.pi * k / 256.0).astype(np.float32), np.sin(2.0 * np.pi * k / 256.0).astype(np.float32)


def axis(n, cells):
    """(cell, t) of the n pixel centres of an axis with `cells` lattice cells; t rounded to fp32."""
    p = np.arange(n, dtype=np.int64)
    num = 2 * p * cells + cells
    return num // (2 * n), ((num % (2 * n)) / float(2 * n)).astype(np.float32)


def lattice_hash(seed, iy, ix):
    """uint32 arithmetic carried in uint64 and masked after every step that can overflow."""
    iy, ix = iy.astype(np.uint64), ix.astype(np.uint64)
    h = (np.uint64(seed) + iy * np.uint64(0x9E3779B1) + ix * np.uint64(0x85EBCA77)) & _M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & _M32
    h ^= h >> np.uint64(16)
    return h


def _noise(seed, h, w, cells_y, cells_x, ft):
    iy, ty = axis(h, cells_y)
    ix, tx = axis(w, cells_x)
    iy, ix = np.broadcast_arrays(iy[:, None], ix[None, :])
    ty, tx = ty.astype(ft)[:, None], tx.astype(ft)[None, :]
    one, six, fifteen, ten = ft(1), ft(6), ft(15), ft(10)

    def fade(t):
        return t * t * t * (t * (t * six - fifteen) + ten)

    gx, gy = gradients()

    def dot(oy, ox, dy, dx):
        k = (lattice_hash(seed, iy + oy, ix + ox) & np.uint64(255)).astype(np.int64)
        return gx[k].astype(ft) * dx + gy[k].astype(ft) * dy

    def lerp(a, b, f):
        return a + f * (b - a)

    fy, fx = fade(ty), fade(tx)
    top = lerp(dot(0, 0, ty, tx), dot(0, 1, ty, tx - one), fx)
    bottom = lerp(dot(1, 0, ty - one, tx), dot(1, 1, ty - one, tx - one), fx)
    return lerp(top, bottom, fy) * (np.float32(np.sqrt(2.0)) if ft is np.float32 else np.sqrt(2.0))


def noise32(seed, h, w, cells_y, cells_x):
    out = _noise(seed, h, w, cells_y, cells_x, np.float32)
    assert out.dtype == np.float32
    return out


def noise64(seed, h, w, cells_y, cells_x):
    return _noise(seed, h, w, cells_y, cells_x, np.float64)


def synthesize(images, desc, masks=None):
    """images fp32 [N, 3, H, W], desc = records with the fields of struct unet_synth_desc -> (corrupted, mask)."""
    n, _, h, w = images.shape
    out = images.copy()
    mask = np.zeros((n, 1, h, w), np.float32) if masks is None else masks.astype(np.float32).copy()
    for i in range(n):
        d = desc[i]
        if not int(d["apply"]):
            continue
        m = noise32(int(d["seed"]), h, w, int(d["cells_y"]), int(d["cells_x"])) > np.float32(d["threshold"])
        donor = np.roll(images[int(d["src"])], (-int(d["shift_y"]), -int(d["shift_x"])), axis=(1, 2))
        donor = donor[list(PERMS[int(d["perm"])])]
        blend = np.float32(d["beta"]) * images[i] + np.float32(d["one_minus_beta"]) * donor
        assert blend.dtype == np.float32
        out[i] = np.where(m[None], blend, images[i])
        mask[i, 0] = np.maximum(mask[i, 0], m.astype(np.float32))
    return out, mask


# ---- the cases of tests/test_gpu_synth.py (tests/test_cpu_synth.py holds the fp32 reference to float64 on the same ones)
# name -> (n, h, w), per-image descriptor fields, whether a mask goes in.  `mixed`: the reference mask must hold both values
# somewhere in the case, so that the blend and the pass-through are both exercised.
def _case(shape, masks=False, mixed=True, **fields):
    return {"shape": shape, "masks": masks, "mixed": mixed, "fields": fields}


CASES = {
    # odd sizes (one pixel per thread: no plane starts 16-byte aligned), an untouched image among applied ones, a mask
    # input, another image as donor and the image itself at the largest shifts
    "odd_17x23": _case((3, 17, 23), masks=True, apply=[1, 0, 1], seed=[11, 12, 13], cells_y=[4, 2, 2], cells_x=[2, 4, 8],
                       threshold=[0.1, 0.1, 0.05], beta=[0.3, 0.5, 0.7], src=[1, 0, 2], shift_y=[3, 0, 16], shift_x=[5, 0, 22],
                       perm=[3, 0, 5]),
    "square_32": _case((2, 32, 32), apply=1, seed=[21, 22], cells_y=[4, 8], cells_x=[8, 2], threshold=[0.2, 0.05],
                       beta=[0.1, 0.8], src=[1, 0], shift_y=[0, 31], shift_x=[1, 0], perm=[1, 2]),
    # 64 cells on an 8-pixel axis: several cells per pixel
    "wide_8x136": _case((1, 8, 136), apply=1, seed=31, cells_y=64, cells_x=8, threshold=0.05, beta=0.4, src=0, shift_y=7,
                        shift_x=135, perm=4),
    "one_cell": _case((2, 16, 16), apply=1, seed=[41, 42], cells_y=1, cells_x=[1, 2], threshold=0.05, beta=0.25, src=[1, 1],
                      shift_y=[0, 15], shift_x=[0, 15], perm=[0, 3]),
    # all six permutations; 12 x 10: the plane is a multiple of 4 pixels, the row is not (16-byte groups cross row ends)
    "perms_12x10": _case((6, 12, 10), masks=True, apply=1, seed=[51, 52, 53, 54, 55, 56], cells_y=[2, 4, 2, 4, 8, 1],
                         cells_x=[4, 2, 2, 8, 4, 2], threshold=0.05, beta=0.5, src=[1, 2, 3, 4, 5, 0], shift_y=[0, 1, 2, 3, 11, 5],
                         shift_x=[9, 0, 2, 3, 4, 5], perm=[0, 1, 2, 3, 4, 5]),
    "empty_and_full": _case((2, 16, 20), apply=1, seed=[61, 62], cells_y=4, cells_x=4, threshold=[2.0, -2.0], beta=0.5,
                            src=[1, 0], shift_y=[1, 2], shift_x=[3, 4], perm=[1, 4]),
    "beta_zero": _case((2, 16, 16), mixed=False, apply=1, seed=[71, 72], cells_y=2, cells_x=4, threshold=-2.0, beta=0.0,
                       src=[1, 0], shift_y=[3, 0], shift_x=[0, 5], perm=[0, 2]),
}
# one case just past the grid cap (2048 blocks x 256 threads x 4 pixels = 32 x 256 x 256): the stride loop's second trip
PAST_CAP = (33, 256, 256)


def past_cap_fields(n=PAST_CAP[0]):
    r = np.random.default_rng(81)
    apply = (r.random(n) < 0.8).astype(int).tolist()
    apply[-1] = 1                            # the image that only the second trip reaches is a corrupted one
    return dict(apply=apply, seed=r.integers(0, 1 << 32, n).tolist(),
                cells_y=(1 << r.integers(0, 7, n)).tolist(), cells_x=(1 << r.integers(0, 7, n)).tolist(), threshold=0.3,
                beta=r.uniform(0.1, 0.8, n).tolist(), src=r.integers(0, n, n).tolist(), shift_y=r.integers(1, 256, n).tolist(),
                shift_x=r.integers(0, 256, n).tolist(), perm=r.integers(0, 6, n).tolist())


def case_inputs(name):
    """(images [N, 3, H, W] fp32, masks [N, 1, H, W] fp32 or None) of a case: seeded, the same in every test."""
    case = CASES[name]
    n, h, w = case["shape"]
    r = np.random.default_rng(sum(name.encode()))
    images = r.standard_normal((n, 3, h, w)).astype(np.float32)
    masks = r.choice(np.array([0.0, 1.0 / 255.0, 1.0], np.float32), (n, 1, h, w), p=[0.7, 0.15, 0.15]) if case["masks"] else None
    return images, masks


def noise_cases():
    """(seed, h, w, cells_y, cells_x, threshold) of every applied image of the GPU cases."""
    out = []
    for name, case in list(CASES.items()) + [("past_cap", {"shape": PAST_CAP, "fields": past_cap_fields()})]:
        n, h, w = case["shape"]
        f = {k: np.broadcast_to(np.asarray(v), (n,)) for k, v in case["fields"].items()}
        out += [(int(f["seed"][i]), h, w, int(f["cells_y"][i]), int(f["cells_x"][i]), float(f["threshold"][i]))
                for i in range(n) if f["apply"][i]]
    return out
