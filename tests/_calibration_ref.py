"""numpy restatement of csrc/calibration.hip (ops.seg_confidence at a temperature, ops.CalibrationMeter): the scaled
confidence in fp32 and float64, the reliability histogram in int64, the temperature sweep in float64 and in an
fp32-per-pixel "host" form that _ref64.assert_measured takes the library functions' error from.
tests/test_cpu_calibration.py pins it, tests/test_gpu_calibration.py holds the device to it."""
import numpy as np

Q_ONE = 65536
U = 2.0 ** -24                                          # one fp32 rounding


def inv_t32(temperature):
    """float32(1 / T), the quotient in float64: what the package hands the kernels"""
    return np.float32(1.0 / float(temperature))


# ---- confidence at a temperature ---------------------------------------------------------------------------------------
def conf_scaled64(logits, inv_t):
    """1 / sum_j exp((z_j - max z) * inv_t) in float64, inv_t the fp32 value the kernel reads"""
    z = np.asarray(logits, np.float64)
    return 1.0 / np.exp((z - z.max(axis=1, keepdims=True)) * np.float64(np.float32(inv_t))).sum(axis=1)


def conf_scaled32(logits, inv_t, subtract_max=True):
    """the kernel's formula in float32 on the host, class by class in order, every operation rounded once"""
    z = np.asarray(logits, np.float32)
    it = np.float32(inv_t)
    best = z.max(axis=1) if subtract_max else np.zeros(z[:, 0].shape, np.float32)
    s = np.zeros(best.shape, np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for j in range(z.shape[1]):
            d = (z[:, j] - best).astype(np.float32)
            s = (s + np.exp((d * it).astype(np.float32)).astype(np.float32)).astype(np.float32)
        return (np.float32(1.0) / s).astype(np.float32)


def conf_scaled_derived(num_classes):
    """The derived terms of the scaled confidence's bound, relative to conf (u = 2^-24): _segvis_ref.conf_bound's
    subtraction (C e^-1 u), additions ((C - 1) u) and division (u), plus the product x_j = d_j * inv_t: one more rounding,
    relative u of x_j and so absolute u |x_j|, which exp turns into u |x_j| e^{x_j} <= u / e of e_j (x_j <= 0); over C
    terms of a sum >= 1: C e^-1 u.  (The subtraction's own error reaches x_j scaled by inv_t, u |d_j| inv_t = u |x_j|:
    the same C e^-1 u as at inv_t = 1.)"""
    c = num_classes
    return c * np.exp(-1.0) * U + (c - 1) * U + U + c * np.exp(-1.0) * U


# ---- reliability histogram ---------------------------------------------------------------------------------------------
def quantise(conf):
    """q(v) = rint(clamp(v, 0, 1) * 65536), ties to even, NaN -> 0: int64"""
    v = np.asarray(conf, np.float32)
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.rint(np.clip(v, np.float32(0), np.float32(1)).astype(np.float64) * 65536.0).astype(np.int64)


def taken_mask(labels, target, num_classes, ignore_index, select):
    """(taken, skipped): skipped = target is ignore_index or outside 0..C-1, or label >= C; select 1 then leaves out the
    pixels whose target and label are both 0 (not skipped: counted nowhere)"""
    lab, t = np.asarray(labels).astype(np.int64), np.asarray(target).astype(np.int64)
    skipped = (t == ignore_index) | (t < 0) | (t >= num_classes) | (lab >= num_classes)
    taken = ~skipped
    if select == 1:
        taken &= ~((t == 0) & (lab == 0))
    return taken, skipped


def histogram(labels, conf, target, num_classes, bins, ignore_index, select):
    """(hist int64 [C][bins][3] = {pixels, correct, sum q} by predicted class and bin, skipped)"""
    lab, t = np.asarray(labels).astype(np.int64).reshape(-1), np.asarray(target).astype(np.int64).reshape(-1)
    q = quantise(conf).reshape(-1)
    taken, skipped = taken_mask(lab, t, num_classes, ignore_index, select)
    b = np.minimum(bins - 1, (q * bins) >> 16)
    hist = np.zeros((num_classes, bins, 3), np.int64)
    l, bb, tt, qq = lab[taken], b[taken], t[taken], q[taken]
    np.add.at(hist[:, :, 0], (l, bb), 1)
    np.add.at(hist[:, :, 1], (l, bb), (tt == l).astype(np.int64))
    np.add.at(hist[:, :, 2], (l, bb), qq)
    return hist, int(skipped.sum())


# ---- temperature sweep -------------------------------------------------------------------------------------------------
def _sweep_pixels(logits, target, ignore_index, select):
    """(z [P, C] float32 of the pixels taken, their targets, non-finite pixels): the non-finite ones are set aside first"""
    z = np.asarray(logits, np.float32)
    n, c = z.shape[:2]
    zp = np.moveaxis(z.reshape(n, c, -1), 1, 2).reshape(-1, c)
    t = np.asarray(target).astype(np.int64).reshape(-1)
    fin = np.isfinite(zp).all(axis=1)
    lab = np.argmax(np.where(fin[:, None], zp, np.float32(0)).astype(np.float64), axis=1)
    taken, _ = taken_mask(lab, t, c, ignore_index, select)
    taken &= fin
    return zp[taken], t[taken], int((~fin).sum())


def sweep64(logits, target, ignore_index, select, inv_t):
    """(nll [K], S [K], counted, nonfinite) in float64: nll[k] = sum over the pixels taken of log(sum_j exp(d_j inv_t[k])) -
    d_t inv_t[k], d_j = z_j - max z; S[k] = the sum of |log sum exp| + |d_t inv_t[k]|, the scale of the comparison"""
    zp, t, nonfinite = _sweep_pixels(logits, target, ignore_index, select)
    d = zp.astype(np.float64) - zp.astype(np.float64).max(axis=1, keepdims=True) if len(zp) else np.zeros((0, 1))
    dt = d[np.arange(len(t)), t] if len(zp) else np.zeros(0)
    nll, scale = [], []
    for it in np.asarray(inv_t, np.float32):
        it = np.float64(it)
        lse = np.log(np.exp(d * it).sum(axis=1)) if len(zp) else np.zeros(0)
        nll.append(float((lse - dt * it).sum()))
        scale.append(float((np.abs(lse) + np.abs(dt * it)).sum()))
    return np.array(nll), np.array(scale), len(t), nonfinite


def sweep32(logits, target, ignore_index, select, inv_t, subtract_max=True):
    """nll [K] with the kernel's per-pixel arithmetic in float32 on the host (every product and sum rounded once, j in
    class order) and the sum over the pixels in float64.  subtract_max=False plants the formula without its max
    subtraction."""
    zp, t, _ = _sweep_pixels(logits, target, ignore_index, select)
    f = np.float32
    if not len(zp):
        return np.zeros(len(inv_t))
    best = zp.max(axis=1) if subtract_max else np.zeros(len(zp), f)
    d = (zp - best[:, None]).astype(f)
    dt = d[np.arange(len(t)), t]
    out = []
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for it in np.asarray(inv_t, f):
            s = np.zeros(len(zp), f)
            for j in range(zp.shape[1]):
                s = (s + np.exp((d[:, j] * it).astype(f)).astype(f)).astype(f)
            term = (np.log(s).astype(f) - (dt * it).astype(f)).astype(f)
            out.append(float(term.astype(np.float64).sum()))
    return np.array(out)
