"""Float64 restatement of the map smoothing (csrc/smooth.hip, evaluation.GaussianSmoother) in numpy: taps, reflect fold,
the W pass and then the H pass, and the error bound the fp32 kernel is held to.  test_cpu_smooth.py pins it to
scipy.ndimage.gaussian_filter(mode="reflect"); nothing here imports the package.

The bound.  K = 2 r + 1 terms per pass, u = 2^-24.  An fp32 evaluation of one pass, in any order and with or without
fused multiply-adds or pairing of the +-k taps, returns sum_k w_k x_k (1 + d_k) with |d_k| <= gamma_K = K u / (1 - K u):
an error of at most gamma_K sum |w_k| |x_k|.  The second pass works on the first one's rounded output, so it passes that
error on through sum |w| (<= gamma_K A, A being both passes applied in float64 to |x| with |w|) and adds its own, at
most gamma_K (1 + gamma_K) A.  Together gamma_K (2 + gamma_K) A <= (2 K + 2) u A for K <= 65 -- against the float64
result computed from the SAME fp32 taps, so the rounding of the taps is on neither side."""
import numpy as np

U = 2.0 ** -24


def radius_of(sigma, truncate=4.0):
    return int(truncate * sigma + 0.5)          # scipy.ndimage's rule


def taps64(sigma, truncate=4.0):
    """taps[k], k = 0 .. r: exp(-0.5 (k / sigma)^2) normalised over the full window, float64."""
    r = radius_of(sigma, truncate)
    if r == 0:
        return np.ones(1)
    k = np.arange(r + 1, dtype=np.float64)
    g = np.exp(-0.5 * (k / sigma) ** 2)
    return g / (g[0] + 2.0 * g[1:].sum())


def fold(i, length):
    """scipy's reflect (d c b a | a b c d | d c b a), folded as often as needed."""
    j = np.mod(np.asarray(i, dtype=np.int64), 2 * length)
    return np.where(j >= length, 2 * length - 1 - j, j)


def window(taps):
    taps = np.asarray(taps)
    return np.concatenate([taps[:0:-1], taps])


def _pass(x, taps, axis, dtype):
    r, length = len(taps) - 1, x.shape[axis]
    xp = np.take(x, fold(np.arange(-r, length + r), length), axis=axis)
    full = window(taps).astype(dtype)
    acc = np.zeros(x.shape, dtype)
    for k in range(2 * r + 1):                  # (one rounding per product and per sum when dtype is float32)
        acc = acc + full[k] * np.take(xp, np.arange(k, k + length), axis=axis)
    return acc


def smooth64(x, taps):
    """[..., H, W] planes: correlation along W, then along H, in float64."""
    x = np.asarray(x, dtype=np.float64)
    return _pass(_pass(x, np.asarray(taps, np.float64), -1, np.float64), np.asarray(taps, np.float64), -2, np.float64)


def smooth32_naive(x, taps32):
    """The same two passes with every product and sum rounded to fp32, left to right: the plainest fp32 kernel."""
    x = np.asarray(x, dtype=np.float32)
    return _pass(_pass(x, np.asarray(taps32, np.float32), -1, np.float32), np.asarray(taps32, np.float32), -2, np.float32)


def bound(x, taps32):
    """(2 K + 2) u A, elementwise."""
    k = 2 * (len(taps32) - 1) + 1
    with np.errstate(invalid="ignore"):
        a = smooth64(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(taps32, np.float64)))
    return (2 * k + 2) * U * a
