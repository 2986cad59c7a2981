"""Float64 references of the bf16 convolution kernels and a comparator that holds them to their rounding.

The kernels read bf16 operands, form exact products, sum them in fp32 and round once on the store.  So a correct
kernel is within half a bf16 ulp of the exact result (bf16-stored outputs), plus an fp32 summation error that is a
small multiple of 2^-24 * S, where S is the sum of |products| behind the element.  The comparator asks for

    bf16-stored:  |out - ref| <= half_ulp_bf16(ref) + 2^-18 * S
    fp32-stored:  |out - ref| <= 2^-18 * S

with ref and S computed in float64 from the bf16-quantised operands.  A dropped or repeated product term, a
mis-zeroed halo element, an epilogue that truncates instead of rounding to nearest-even or a missing split-K slab
moves an element by far more than that; the max|ref|-relative bound of check() in test_gpu_kernels.py does not see
them.  Plain helper module: the GPU tests and the CPU self-test (test_cpu_ref64.py) import it.

The convolution references take the compute dtype of the kernel under test (dtype=, default bf16) and read their
operands with rd().  The fp32 kernels (the "parity" mode: conv3_kernel<float>, igemm_kernel<float>, wgrad_kernel<float>)
store fp32, so they are held to 2^-18 S alone, on UNROUNDED fp32 operands: an fp32 kernel reads every bit of its inputs,
and inputs that already lie on the bf16 grid would hide a kernel that narrows its operands on the way to the matrix
unit (bf16 or a 10-bit mantissa move an element by 30 to 200 bounds, test_cpu_ref64.py).
"""
import torch
import torch.nn.functional as F

SUM_EPS = 2.0 ** -18          # fp32 summation allowance, relative to S (64 x the 2^-24 of one fp32 rounding)
BF16_MANT = 8                 # bf16 significand bits (7 stored + the implicit one)

# the largest weight-gradient reduction length (N * H * W pixels) any bf16 test in the suite compares with the fp32
# bound: BIG_CONV_CASES (8, 128, 128, 128, 128) of test_gpu_kernels.py.  test_cpu_ref64.py plants a missing 32-pixel
# block at this K; the GPU tests assert they stay at or below it.
MAX_WGRAD_K = 8 * 128 * 128

# Reductions over pixels (BatchNorm statistics, dbeta / dgamma): the longest one the suite holds to 2^-18 S is the
# benchmark's 32 x 256 x 256.  One missing 32-pixel row group moves a sum by about 32 |mean| (+ noise 6 sigma), the
# bound at that length is 2^-18 * 2 097 152 * E|y| = 8 E|y|: such a defect is only visible when the channel has an offset.
# The large GPU cases therefore give y and the gradient per-channel offsets of at least MIN_STREAM_OFFSET sigma;
# test_cpu_ref64.py plants the defect at MAX_STREAM_PIXELS with exactly that offset, the GPU tests assert both limits.
MAX_STREAM_PIXELS = 32 * 256 * 256
MIN_STREAM_OFFSET = 1.0

# worst err / bound seen per comparator kind in this process (printed by the tests, quoted in reviews)
WORST = {"bf16": 0.0, "fp32": 0.0}


def q64(t):
    """the value a bf16 kernel reads: round to bf16, then exact in float64"""
    return t.detach().to(torch.bfloat16).to(torch.float64).cpu()


def half_ulp_bf16(ref):
    """half a bf16 ulp at |ref|, exact from the binade of ref (0 where ref == 0: the S term covers cancellation)"""
    ref = ref.to(torch.float64)
    _, e = torch.frexp(ref)                          # |ref| in [2^(e-1), 2^e): ulp = 2^(e-1-7)
    h = torch.ldexp(torch.ones_like(ref), (e - 1 - BF16_MANT).to(torch.int32))
    return torch.where(ref == 0, torch.zeros_like(ref), h)


def round_bf16_toward_zero(x):
    """bf16 rounding by truncation of the fp32 bit pattern (a defective epilogue, for the self-test)"""
    b = x.to(torch.float32).contiguous().view(torch.int32) & ~0xFFFF
    return b.view(torch.float32).to(torch.bfloat16)


# ------------------------------------------------------------------ references: (value, magnitude S) in float64
def conv3x3(x, w, dtype=torch.bfloat16):
    """y = conv2d(x, w, padding=1)"""
    x, w = rd(x, dtype), rd(w, dtype)
    return F.conv2d(x, w, padding=1), F.conv2d(x.abs(), w.abs(), padding=1)


def conv3x3_dgrad(dy, w, dtype=torch.bfloat16):
    """dx of y = conv2d(x, w, padding=1)"""
    dy, w = rd(dy, dtype), rd(w, dtype)
    return F.conv_transpose2d(dy, w, padding=1), F.conv_transpose2d(dy.abs(), w.abs(), padding=1)


def conv3x3_wgrad(x, dy, dtype=torch.bfloat16):
    """dw of y = conv2d(x, w, padding=1), dw[co, ci, ky, kx]"""
    x, dy = rd(x, dtype), rd(dy, dtype)
    shape = (dy.shape[1], x.shape[1], 3, 3)
    g = torch.nn.grad.conv2d_weight
    return g(x, shape, dy, padding=1), g(x.abs(), shape, dy.abs(), padding=1)


def convt2x2(x, w, b, dtype=torch.bfloat16):
    """y = conv_transpose2d(x, w, b, stride=2); x and w[ci, co, 2, 2] read in the compute dtype, the bias stays fp32"""
    x, w, b = rd(x, dtype), rd(w, dtype), b.detach().to(torch.float64).cpu()
    return F.conv_transpose2d(x, w, b, stride=2), F.conv_transpose2d(x.abs(), w.abs(), b.abs(), stride=2)


def convt2x2_dgrad(dy, w, dtype=torch.bfloat16):
    """dx of y = conv_transpose2d(x, w, stride=2)"""
    dy, w = rd(dy, dtype), rd(w, dtype)
    return F.conv2d(dy, w, stride=2), F.conv2d(dy.abs(), w.abs(), stride=2)


def convt2x2_wgrad(x, dy, dtype=torch.bfloat16):
    """(dw[ci, co, 2, 2], db[co]) of y = conv_transpose2d(x, w, b, stride=2)"""
    x, dy = rd(x, dtype), rd(dy, dtype)
    n, ci, h, w_ = x.shape
    co = dy.shape[1]
    d = dy.view(n, co, h, 2, w_, 2)

    def wg(a, g):
        return torch.einsum("nihw,nohywx->ioyx", a, g)
    return (wg(x, d), wg(x.abs(), d.abs())), (dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3)))


def bn_relu_mask(y, scale, shift, tie=1e-4):
    """(on, clear): the ReLU mask [scale*y + shift > 0] of the fused BatchNorm backward, and where it is decided away
    from rounding level (|scale*y + shift| > tie) -- elements outside `clear` are left out of the comparison"""
    z = torch.addcmul(shift.double()[None, :, None, None], q64(y), scale.double()[None, :, None, None])
    return z > 0, z.abs() > tie


def sums_over_pixels(v):
    """per-channel (sum, S) over an NCHW tensor, float64"""
    v = v.detach().to(torch.float64).cpu()
    return v.sum((0, 2, 3)), v.abs().sum((0, 2, 3))


# ------------------------------------------------------------------ streaming / reduction kernels: (value, S) in float64
# These references take the compute dtype of the kernel under test: rd() gives the operands the kernel reads.
def rd(t, dtype):
    """the value a kernel of compute dtype `dtype` reads, exact in float64"""
    return t.detach().to(dtype).to(torch.float64).cpu()


def stored(v, dtype):
    """a float64 value as a correct kernel stores it: rounded once to fp32 (the register), then to the compute dtype"""
    return v.to(torch.float32).to(dtype).to(torch.float64)


def _c(v):
    return v.detach().to(torch.float64).cpu()[None, :, None, None]


def _eps32(eps):
    return float(torch.tensor(eps, dtype=torch.float32))


def bn_train_stats(y, dtype, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5):
    """unet_bn_train_stats / unet_bn_finalize_partials: every output as (value, S) with SUM_EPS * S the DERIVED bound.

    The kernel sums y and y^2 (|d sum y| <= SUM_EPS sum|y|, |d sum y^2| <= SUM_EPS sum y^2), everything after that is
    fp64 until the fp32 store.  With M pixels:
      mean    d_mean  = SUM_EPS E|y| + 2^-24 |mean|                              (sum error / M, one fp32 store)
      var     d       = SUM_EPS (E[y^2] + 2 |mean| E|y|)                         (var = E[y^2] - mean^2)
      istd    d_istd  = istd (d / (2 (var + eps)) + 2^-23)                        (d/dvar (var+eps)^-1/2, store + fp32 eps)
      scale   d_scale = |gamma| d_istd + 2^-24 |scale|                           (product rule, one fp32 product)
      shift   d_shift = |scale| d_mean + |mean| d_scale + 2^-23 (|beta| + |mean scale|)   (fma of the ROUNDED mean)
      running mean / var = (1 - m) old + m new in fp32: m d_new + 2^-22 (|(1 - m) old| + |m new|)   (four fp32 roundings:
              1 - m, two products, the sum), new variance = var M / (M - 1) (var itself when M = 1) with d M / (M - 1).
    momentum=None of nn.BatchNorm2d is the caller passing 1 / num_batches_tracked as the momentum.
    Also returns 'istd_rel' = d_istd / istd per channel (the allowed relative error the tests print)."""
    y = rd(y, dtype)
    M = y.numel() // y.shape[1]
    g, b = gamma.detach().double().cpu(), beta.detach().double().cpu()
    eps = _eps32(eps)
    ea, ey2 = y.abs().mean((0, 2, 3)), (y * y).mean((0, 2, 3))
    mean = y.mean((0, 2, 3))
    var = ((y - mean[None, :, None, None]) ** 2).mean((0, 2, 3))           # two-pass: no cancellation in the reference
    d_mean = SUM_EPS * ea + 2.0 ** -24 * mean.abs()
    d = SUM_EPS * (ey2 + 2 * mean.abs() * ea)
    istd = (var + eps).rsqrt()
    d_istd = istd * (d / (2 * (var + eps)) + 2.0 ** -23)
    scale = g * istd
    d_scale = g.abs() * d_istd + 2.0 ** -24 * scale.abs()
    shift = b - mean * scale
    d_shift = scale.abs() * d_mean + mean.abs() * d_scale + 2.0 ** -23 * (b.abs() + (mean * scale).abs())
    out = {"mean": (mean, d_mean / SUM_EPS), "istd": (istd, d_istd / SUM_EPS), "scale": (scale, d_scale / SUM_EPS),
           "shift": (shift, d_shift / SUM_EPS), "var": (var, d / SUM_EPS), "istd_rel": d_istd / istd}
    if running_mean is not None:
        m = float(torch.tensor(momentum, dtype=torch.float32))
        rm, rv = running_mean.detach().double().cpu(), running_var.detach().double().cpu()
        k = M / (M - 1.0) if M > 1 else 1.0
        unb = var * k
        nrm, nrv = (1 - m) * rm + m * mean, (1 - m) * rv + m * unb
        d_rm = m * d_mean + 2.0 ** -22 * (((1 - m) * rm).abs() + (m * mean).abs())
        d_rv = m * (d * k + 2.0 ** -24 * unb) + 2.0 ** -22 * (((1 - m) * rv).abs() + (m * unb).abs())
        out["running_mean"], out["running_var"] = (nrm, d_rm / SUM_EPS), (nrv, d_rv / SUM_EPS)
    return out


def bn_relu_apply(y, dtype, scale, shift):
    """unet_bn_relu_apply (scale / shift from unet_bn_eval_coeffs or the test): a = max(y scale + shift, 0)"""
    y = rd(y, dtype)
    t = y * _c(scale)
    return (t + _c(shift)).clamp_min(0), t.abs() + _c(shift).abs()


def fold_weight(w, scale):
    """the folded weight of an eval-mode conv + BatchNorm layer as unet_pack_conv_weight_folded(_seg) forms it: ONE fp32
    product w * scale[co] (no fma), fp32"""
    return w.detach().float().cpu() * scale.detach().float().cpu()[:, None, None, None]


def conv3x3_bias_relu(x, w, scale, shift, dtype, relu=True):
    """unet_conv3x3_bias_relu on the folded weights (inference, BatchNorm(eval) folded into the layer):
    value = max(conv(x, fold_weight(w, scale)) + shift, 0) with the folded weight and x read in the compute dtype and
    the shift in fp32; S = conv(|x|, |w_folded|) + |shift|.  ReLU is 1-Lipschitz, so the bound of the plain convolution
    holds behind it: half a bf16 ulp + 2^-18 S (assert_bf16), 2^-18 S for fp32 (assert_fp32).  scale / shift: as
    unet_bn_eval_coeffs returned them (read back from the device -- the coefficient kernel has its own test, and its
    rounding stays out of this bound).  x: one tensor, or the already concatenated / centre-padded pair.
    relu=False: the entry point's relu = 0."""
    xq, wq = rd(x, dtype), rd(fold_weight(w, scale), dtype)
    sh = _c(shift)
    v = F.conv2d(xq, wq, padding=1) + sh
    S = F.conv2d(xq.abs(), wq.abs(), padding=1) + sh.abs()
    return (v.clamp_min(0) if relu else v), S


def bn_eval_coeffs(gamma, beta, running_mean, running_var, eps=1e-5):
    """unet_bn_eval_coeffs(4): istd = (running_var + eps)^-1/2 (fp64, one fp32 store), scale = gamma istd, shift = beta -
    running_mean scale (fp32): bounds as in bn_train_stats with exact statistics (d = d_mean = 0)."""
    g, b = gamma.detach().double().cpu(), beta.detach().double().cpu()
    rm, rv = running_mean.detach().double().cpu(), running_var.detach().double().cpu()
    istd = (rv + _eps32(eps)).rsqrt()
    d_istd = 2.0 ** -23 * istd
    scale = g * istd
    d_scale = g.abs() * d_istd + 2.0 ** -24 * scale.abs()
    shift = b - rm * scale
    d_shift = rm.abs() * d_scale + 2.0 ** -23 * (b.abs() + (rm * scale).abs())
    return {"mean": (rm, torch.zeros_like(rm)), "istd": (istd, d_istd / SUM_EPS), "scale": (scale, d_scale / SUM_EPS),
            "shift": (shift, d_shift / SUM_EPS)}


def bn_bwd_premasked(dz, y, dtype, gamma, mean, istd, frozen=False):
    """The BatchNorm backward for a gradient that carries the ReLU mask already (dz, y: as the kernel reads them):
    dbeta = sum dz, dgamma = sum dz yhat (yhat = (y - mean) istd), dy = A dz + B y + K with A = gamma istd,
    B = -A istd dgamma / M, K = -A dbeta / M - B mean (frozen statistics: B = K = 0).
    S of dy: |A dz| for its own product, plus what the kernel's own dgamma / dbeta may be off by, carried through B and K:
    |A| istd S_dgamma / M (|y| + |mean|) + |A| S_dbeta / M.  S_dgamma >= |dgamma|, so this also covers the fp32 roundings
    of the coefficients and the cancellation of B y against K for a channel whose mean is large against its spread."""
    dz, y = rd(dz, dtype), rd(y, dtype)
    M = y.numel() // y.shape[1]
    mu, si, A = _c(mean), _c(istd), _c(gamma) * _c(istd)
    t = dz * ((y - mu) * si)
    db, sdb = dz.sum((0, 2, 3)), dz.abs().sum((0, 2, 3))
    dg, sdg = t.sum((0, 2, 3)), t.abs().sum((0, 2, 3))
    if frozen:
        dy, S = A * dz, (A * dz).abs()
    else:
        B = -A * si * dg[None, :, None, None] / M
        K = -A * db[None, :, None, None] / M - B * mu
        dy = A * dz + B * y + K
        S = (A * dz).abs() + A.abs() * si * sdg[None, :, None, None] / M * (y.abs() + mu.abs()) \
            + A.abs() * sdb[None, :, None, None] / M
    return {"dbeta": (db, sdb), "dgamma": (dg, sdg), "dy": (dy, S)}


def bn_relu_bwd(da, y, dtype, gamma, mean, istd, scale, shift, frozen=False, mask_ge=False):
    """unet_bn_relu_bwd / _frozen: dz = da [y scale + shift > 0], then bn_bwd_premasked.  The sign of the fp32
    fma(y, scale, shift) is the sign of the exact value (a rounding never crosses zero), so the mask of the sums is exact;
    'clear' (bn_relu_mask) is for the element-wise dy comparison only.  mask_ge: the defective mask [z >= 0]."""
    yq, daq = rd(y, dtype), rd(da, dtype)
    z = yq * _c(scale) + _c(shift)
    on = (z >= 0) if mask_ge else (z > 0)
    dz = daq * on
    out = bn_bwd_premasked(dz, yq, torch.float64, gamma, mean, istd, frozen)
    out["dz"], out["on"], out["clear"] = (dz, dz.abs()), on, (z.abs() > 1e-4) | (z == 0)      # (an exact zero is no tie)
    return out


def maxpool2(x):
    """MaxPool2d(2), floor: exact (no rounding freedom, compare with torch.equal)"""
    return F.max_pool2d(x.detach().to(torch.float64).cpu(), 2)


def maxpool2_route(x, g, last=False):
    """gradient of MaxPool2d(2): g goes to the FIRST maximum of each window in row-major order (last=True: the defect),
    rows / columns dropped by the floor get 0.  x, g float64.  Returns the routed gradient (exact: one term per element)."""
    n, c, h, w = x.shape
    oh, ow = h // 2, w // 2
    win = x[:, :, :2 * oh, :2 * ow].reshape(n, c, oh, 2, ow, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, oh, ow, 4)
    eq = win == win.max(-1, keepdim=True).values
    if last:
        eq = eq.flip(-1)
    first = eq & (eq.cumsum(-1) == 1)
    if last:
        first = first.flip(-1)
    r = (first * g[..., None]).reshape(n, c, oh, ow, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, 2 * oh, 2 * ow)
    return F.pad(r, [0, w - 2 * ow, 0, h - 2 * oh])


def bn_relu_pool_bwd(y, dpooled, da_old, dtype, scale, shift, mean):
    """unet_bn_relu_pool_bwd: da = da_old + route(dpooled) with the route taken on the activation AS STORED (a rounded to
    the compute dtype: ties between stored values go to the first), stored once; dz = da [z > 0] on the fp32
    pre-activation; the two sums run over the STORED dz: sum dz, sum dz (y - mean).
    -> {'dz': (value, S), 'dz_stored', 'sum': (.., S), 'sum_c': (.., S)}"""
    yq, g = rd(y, dtype), rd(dpooled, dtype)
    old = rd(da_old, dtype) if da_old is not None else torch.zeros_like(yq)
    z = yq * _c(scale) + _c(shift)
    routed = maxpool2_route(stored(z.clamp_min(0), dtype), g)
    on = z > 0
    da = old + routed
    dzs = stored(da, dtype) * on
    t = dzs * (yq - _c(mean))
    return {"dz": (da * on, (old.abs() + routed.abs()) * on), "dz_stored": dzs, "on": on,
            "sum": (dzs.sum((0, 2, 3)), dzs.abs().sum((0, 2, 3))), "sum_c": (t.sum((0, 2, 3)), t.abs().sum((0, 2, 3)))}


def bilinear_weights(n_in, wrong=False):
    """[2 n_in][n_in] interpolation matrix of nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True) in
    float64: source coordinate o (n_in - 1) / (2 n_in - 1) (wrong=True: n_in / (2 n_in), the defect)"""
    n_out = 2 * n_in
    o = torch.arange(n_out, dtype=torch.float64)
    src = o * ((n_in / n_out) if wrong else ((n_in - 1) / (n_out - 1)))
    i0 = src.floor().clamp_max(n_in - 1).long()
    i1 = (i0 + 1).clamp_max(n_in - 1)
    f = src - i0
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    m.scatter_add_(1, i0[:, None], (1 - f)[:, None])
    m.scatter_add_(1, i1[:, None], f[:, None])
    return m


def bilinear2x(x, dtype, wrong=False):
    """unet_upsample_bilinear2x_fwd: weighted sum of the four neighbours, S = the same sum of |.| (weights >= 0)"""
    x = rd(x, dtype)
    wy, wx = bilinear_weights(x.shape[2], wrong), bilinear_weights(x.shape[3], wrong)
    f = lambda v: torch.einsum("oh,nchw,pw->ncop", wy, v, wx)       # noqa: E731
    return f(x), f(x.abs())


def bilinear2x_bwd(dy, dtype):
    """unet_upsample_bilinear2x_bwd: the adjoint"""
    dy = rd(dy, dtype)
    wy, wx = bilinear_weights(dy.shape[2] // 2), bilinear_weights(dy.shape[3] // 2)
    f = lambda v: torch.einsum("oh,ncop,pw->nchw", wy, v, wx)       # noqa: E731
    return f(dy), f(dy.abs())


def adam_step(p, g, m, v, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=False,
              grad_scale=1.0, bias_step=None, swap_decay=False):
    """one step of torch.optim.Adam (L2 decay joins the gradient) / AdamW (decoupled: p *= 1 - lr wd first) in float64
    from the state given.  -> ((p, S), (m, S), (v, S)); S = |value| + the absolute terms it was formed from.
    bias_step / swap_decay (the other decay rule): the planted defects of test_cpu_ref64.py."""
    p, g, m, v = (t.detach().to(torch.float64).cpu() for t in (p, g, m, v))
    lr, eps, wd = (float(torch.tensor(x, dtype=torch.float32)) for x in (lr, eps, weight_decay))
    g = g * grad_scale
    sp = p.abs()
    if decoupled != swap_decay:
        p = p * (1 - lr * wd)
    else:
        g = g + wd * p
    m2 = beta1 * m + (1 - beta1) * g
    v2 = beta2 * v + (1 - beta2) * g * g
    t = step if bias_step is None else bias_step
    bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
    upd = lr / bc1 * m2 / (v2.sqrt() / bc2 ** 0.5 + eps)
    p2 = p - upd
    return ((p2, p2.abs() + sp + upd.abs()), (m2, m2.abs() + (beta1 * m).abs() + ((1 - beta1) * g).abs()),
            (v2, 2 * v2))


def anomaly_score(recon, image, l1=False):
    """unet_anomaly_score: score = mean_c (recon - image)^2 (l1: mean_c |.|) per pixel, image_score = its mean over the
    pixels.  S: the same with |recon| + |image| for the difference (the subtraction is rounded relative to its operands).
    -> ((score, S), (image_score, S))"""
    r, i = recon.detach().double().cpu(), image.detach().double().cpu()
    d, a = r - i, r.abs() + i.abs()
    v, S = (d.abs(), a) if l1 else (d * d, a * a)
    v, S = v.mean(1), S.mean(1)
    return (v, S), (v.flatten(1).mean(1), S.flatten(1).mean(1))


def mse_focal(recon, image, amap, mask, alpha=0.25, gamma=2.0):
    """unet_loss_mse_focal, the oracle's formula (oracle/unet_oracle.py combined_loss / focal_loss / _BCE) in float64,
    clamps included: mse = mean d^2, d_recon = 2 d / n; bce = -(t max(log p, -100) + (1 - t) max(log(1 - p), -100)),
    pt = exp(-bce), focal = mean alpha (1 - pt)^gamma bce, d_amap = alpha ((1 - pt)^gamma + gamma (1 - pt)^(gamma - 1) pt bce)
    (p - t) / max((1 - p) p, 1e-12) / n.  S = |value| + the absolute terms it was formed from: 1 - pt is formed from 1 and
    pt, so S carries (1 + pt) in its place; d carries |recon| + |image|."""
    r, i = recon.detach().double().cpu().reshape(-1), image.detach().double().cpu().reshape(-1)
    p, t = amap.detach().double().cpu().reshape(-1), mask.detach().double().cpu().reshape(-1)
    d, a = r - i, r.abs() + i.abs()
    bce = -(t * p.log().clamp_min(-100.0) + (1 - t) * (1 - p).log().clamp_min(-100.0))
    pt = (-bce).exp()
    om, op = 1 - pt, 1 + pt
    dbce = (p - t) / ((1 - p) * p).clamp_min(1e-12)
    na = p.numel()

    def dfoc(x):
        return alpha * (x ** gamma + gamma * x ** (gamma - 1) * pt * bce) * dbce / na
    return {"mse": ((d * d).mean(), (a * a).mean()), "d_recon": (2 * d / d.numel(), 2 * a / d.numel()),
            "focal": ((alpha * om ** gamma * bce).mean(), (alpha * op ** gamma * bce).mean()),
            "d_amap": (dfoc(om), dfoc(op).abs())}


def head_fwd(x, dtype, weight, bias, sigmoid):
    """unet_head_fwd: out = conv1x1(x, w) + b (fp32 NCHW), optionally through a sigmoid.  Logits: S = sum |x w| + |b|.
    Probabilities s: S = s + s (1 - s) S_logit (the value, plus what the logit's summation error becomes behind the
    sigmoid's slope); the sigmoid itself is a library function -> assert_measured(extra=SUM_EPS)."""
    x, w, b = rd(x, dtype), weight.detach().double().cpu(), bias.detach().double().cpu()
    z, S = F.conv2d(x, w, b), F.conv2d(x.abs(), w.abs(), b.abs())
    if not sigmoid:
        return z, S
    s = torch.sigmoid(z)
    return s, s + s * (1 - s) * S


def head_bwd(x, dtype, out, dout, weight, sigmoid):
    """unet_head_bwd from the forward result `out` and its gradient `dout` as the kernel reads them (fp32): dlogit = dout
    out (1 - out) with a sigmoid, dout without; dx = sum_co dlogit w (compute dtype), dW = sum_pixels dlogit x, db = sum_pixels
    dlogit (fp32).  S: the sums of the absolute products.  -> {'dx', 'dw', 'db'}"""
    x, w = rd(x, dtype), weight.detach().double().cpu()
    o, g = out.detach().double().cpu(), dout.detach().double().cpu()
    dl = g * o * (1 - o) if sigmoid else g
    w2 = w.flatten(1)
    return {"dx": (torch.einsum("nohw,oi->nihw", dl, w2), torch.einsum("nohw,oi->nihw", dl.abs(), w2.abs())),
            "dw": (torch.einsum("nohw,nihw->oi", dl, x)[:, :, None, None], torch.einsum("nohw,nihw->oi", dl.abs(), x.abs())[:, :, None, None]),
            "db": (dl.sum((0, 2, 3)), dl.abs().sum((0, 2, 3)))}


def head_bnrelu_fwd(y, dtype, scale, shift, weight, bias, sigmoid):
    """unet_head_bnrelu_fwd: the 1x1 head on a = max(y scale + shift, 0) formed on load and rounded to the compute dtype
    like the stored activation of the unfused pair -- bn_relu_apply, stored, then head_fwd."""
    a = stored(bn_relu_apply(y, dtype, scale, shift)[0], dtype)
    return head_fwd(a, torch.float64, weight, bias, sigmoid)


def head_bnrelu_bwd(y, dtype, scale, shift, mean, out, dout, weight, sigmoid):
    """unet_head_bnrelu_bwd: head_bwd on the recomputed, rounded activation (dW, db); dz = dx [y scale + shift > 0] stored
    once in the compute dtype; the BatchNorm-backward partials are sums over the STORED dz: sum dz, sum dz (y - mean).
    -> {'dw', 'db', 'dz', 'dz_stored', 'sum', 'sum_c'}"""
    yq = rd(y, dtype)
    z = yq * _c(scale) + _c(shift)
    hb = head_bwd(stored(z.clamp_min(0), dtype), torch.float64, out, dout, weight, sigmoid)
    on = z > 0
    dzs = stored(hb["dx"][0], dtype) * on
    t = dzs * (yq - _c(mean))
    return {"dw": hb["dw"], "db": hb["db"], "dz": (hb["dx"][0] * on, hb["dx"][1] * on), "dz_stored": dzs,
            "sum": (dzs.sum((0, 2, 3)), dzs.abs().sum((0, 2, 3))), "sum_c": (t.sum((0, 2, 3)), t.abs().sum((0, 2, 3)))}


def ssim(img1, img2, window=11, per_image=False):
    """unet_ssim_loss (per_image: unet_ssim_loss_per_image), the oracle's formula (oracle/unet_oracle.py ssim_loss) in
    float64: depthwise Gaussian blur with zero padding, variances as E[x^2] - mu^2, C1 = 1e-4, C2 = 9e-4,
    loss = 1 - mean(map) over everything, or per image.  The gradient is the blur of the five adjoint maps
    M = d loss / d (mu1, mu2, E11, E22, E12):  d img1 = blur(M_mu1) + 2 img1 blur(M_E11) + img2 blur(M_E12), d img2 alike.
    S of a gradient: the same expression over |M| and |img|; S of a loss: 1 + mean |map|.
    -> {'loss': (v, S), 'd1': (v, S), 'd2': (v, S)}"""
    from oracle import unet_oracle as O
    x, y = img1.detach().double().cpu(), img2.detach().double().cpu()
    c = x.shape[1]
    win = O.gaussian_window(window, 1.5, torch.float64)[None, None].expand(c, 1, -1, -1).contiguous()

    def blur(t):
        return F.conv2d(t, win, padding=window // 2, groups=c)
    lv = [blur(t).requires_grad_(True) for t in (x, y, x * x, y * y, x * y)]
    mu1, mu2, e11, e22, e12 = lv
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    smap = ((2 * mu1 * mu2 + c1) * (2 * (e12 - mu1 * mu2) + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (e11 - mu1 * mu1 + e22 - mu2 * mu2 + c2))
    if per_image:
        loss, sl = 1 - smap.mean((1, 2, 3)), 1 + smap.abs().mean((1, 2, 3))
    else:
        loss, sl = 1 - smap.mean(), 1 + smap.abs().mean()
    m1, m2, m11, m22, m12 = torch.autograd.grad(loss.sum(), lv)
    d1 = blur(m1) + 2 * x * blur(m11) + y * blur(m12)
    d2 = blur(m2) + 2 * y * blur(m22) + x * blur(m12)
    s1 = blur(m1.abs()) + 2 * x.abs() * blur(m11.abs()) + y.abs() * blur(m12.abs())
    s2 = blur(m2.abs()) + 2 * y.abs() * blur(m22.abs()) + x.abs() * blur(m12.abs())
    return {"loss": (loss.detach(), sl.detach()), "d1": (d1, s1), "d2": (d2, s2)}


# ------------------------------------------------------------------ segmentation loss (csrc/segloss.hip)
# The largest sizes at which the GPU tests (test_gpu_segloss.py) rely on the comparator to see each class of defect;
# test_cpu_ref64.py plants the defect at exactly these sizes, the GPU tests assert they stay within them.
#   one block's partial (4096 pixels) missing: moves a per-image sum by 4096 / hw and the CE denominator by 4096 / (N hw),
#     both far above 2^-18 at every size in use -- planted at the largest image and the largest batch;
#   one pixel missing at the tail: moves a per-image sum by about 1 / hw, which reaches the 2^-18 bound near 512 x 512 --
#     only the small pixel-count sweep is relied on for it.
MAX_SEG_IMAGE_HW = 1408 * 1024
MAX_SEG_PIXELS = 48 * 512 * 512
MAX_SEG_TAIL_HW = 12289
MAX_SEG_TAIL_HW_C1 = 257      # one class: the gradient is identically 0, only the (nearly flat) Dice value is left to see it
SEG_CE_ABS = 2.0 ** -24       # see seg_loss: what an fp32 sum / probability next to 1 cannot resolve
SEG_BLOCK = 4096              # pixels per block of seg_reduce_kernel below its cap on blocks per image

SEG_DEFECTS = ("drop_block", "drop_tail", "b_sign", "a_class", "no_focal_dterm", "ce_clamp", "sump_skips_ignored",
               "focal_over_valid")


def _f32(x):
    return float(torch.tensor(float(x), dtype=torch.float32))


def _seg_pixels(z, t, C, ignore, cw, alpha, gamma, dtype, is_prob=False, defect=None):
    """per-pixel quantities of ONE image ([C, P] logits, [P] labels) evaluated in `dtype`: float64 is the reference,
    float32 the host evaluation of the same formulas that assert_measured holds the device functions against"""
    z = z.to(dtype)
    P = z.shape[1]
    valid = (t != ignore) & (t >= 0) & (t < C)
    tc = torch.where(valid, t, torch.zeros_like(t))
    h = torch.zeros((C, P), dtype=torch.bool).scatter_(0, tc[None], valid[None])
    if is_prob:
        return {"p": z, "h": h, "valid": valid, "tc": tc}
    d = z - z.max(0).values                              # <= 0, exactly 0 at the maximum
    e = d.exp()
    s = e.sum(0)
    p = e / s
    dt = d.gather(0, tc[None])[0]
    nll = torch.where(valid, s.log() - dt, torch.zeros_like(s))
    if defect == "ce_clamp":                             # -log(max(pt, 1e-38)) of a normalised probability
        nll = nll.clamp_max(87.498)
    pt = torch.where(valid, p.gather(0, tc[None])[0], torch.ones_like(s))
    w = torch.where(valid, (cw.to(dtype)[tc] if cw is not None else torch.ones_like(s)), torch.zeros_like(s))
    om = 1 - pt
    foc = torch.where(valid, alpha * om ** gamma * nll, torch.zeros_like(s))
    return {"p": p, "h": h, "valid": valid, "tc": tc, "d": d, "nll": nll, "pt": pt, "w": w, "om": om, "foc": foc,
            "s_nll": torch.where(valid, s.log() + dt.abs(), torch.zeros_like(s))}


def seg_loss(logits, target, class_weights=None, ignore_index=-1, ce_w=1.0, dice_w=1.0, focal_w=0.0, alpha=1.0,
             gamma=2.0, is_prob=False, grad=True, defect=None, images=None):
    """unet_seg_loss in float64 from the fp32 logits [N, C, hw] and int64 labels [N, hw] the kernel reads.

    CONTRACT (wider than the reference's F.cross_entropy / dice_loss / focal_loss):
      * a label equal to ignore_index, negative or >= C is not valid: it adds nothing to CE, focal, the Dice intersection I
        and the one-hot sum T; its softmax probability still enters the Dice sum P = sum p;
      * CE = sum w nll / sum w over valid pixels, 0 with a zero CE gradient when sum w = 0 (torch: NaN);
      * focal = sum alpha (1 - pt)^gamma nll / (N hw): a mean over ALL pixels;
      * Dice: dice[n, c] = (2 I + s) / (P + T + s), s = 1e-8, loss = 1 - mean over N C;
      * total = the terms whose weight is > 0, weighted;  is_prob: Dice of the given map, gradient w.r.t. the map.
    Gradient, closed form:  d = p_c (g_c - sum_j g_j p_j) + k (p_c - h_c),  g_c = h_c A_c + B_c,
      A = -dice_w 2 / (N C U),  B = dice_w (2 I + s) / (N C U^2),  U = P + T + s,
      k = ce_w w / sum w + focal_w alpha ((1 - pt)^gamma + gamma (1 - pt)^(gamma - 1) pt nll) / (N hw).

    BOUNDS.  Every output is (value, S) plus an absolute allowance; assert_measured(..., absolute=) asks for
        |out - ref| <= S (max(4 host, 2^-22) + extra) + absolute,
    host = the worst |fp32 host evaluation - ref| / S of the same formulas (exp, log, pow and the softmax division are
    library functions: the module's measured rule; the host evaluation is never the kernel).
    Per pixel:
      p_c    = exp(d_c) / sum exp(d), d = z - max z.  The fp32 subtraction rounds d by 2^-24 |d|, which exp turns into a
               RELATIVE error 2^-24 |d| = 2^-22 |d| / 4 of p_c:  S(p_c) = p_c (1 + |d_c| / 4).
      nll    = log(sum) - d_t:  S = log(sum) + |d_t| (both roundings are relative to their own term), plus the absolute
               SEG_CE_ABS = 2^-24: the sum is an fp32 number in [1, C] whose largest term is exactly 1, half an ulp of it
               next to 1 is 2^-24 and d log(sum) = d sum / sum, so an nll below that cannot be resolved (the same
               half ulp of pt at 1 in the -log(pt) form).  Derived, not measured.
      1 - pt   is formed from 1 and pt: S carries (1 + pt) in its place (mse_focal's convention), so
      focal_i  S = alpha (1 + pt)^gamma S(nll), absolute alpha (1 + pt)^gamma 2^-24.
    Sums of like-signed fp32 terms (I, P, CE numerator and denominator, focal) add SUM_EPS S; T is a count, exact.
    First-order propagation (sums are fp64 after the per-block fp32 partials, every store is one fp32 rounding):
      r_I, r_P = SUM_EPS + lib: relative error of I and P, lib = max(4 x measured host error of the sum, 2^-22)
      dice[n,c]  d = 2 r_I I / U + dice r_P P / U                    -> dice loss: S = 1 + mean(2 I / U + dice P / U)
      A          r_A = r_P P / U + 2^-24                              (d(1 / U) = dU / U^2, one store)
      B          r_B = r_I 2 I / (2 I + s) + 2 r_P P / U + 2^-24      (d(1 / U^2) = 2 dU / U^3)
      ce         S = sum w S(nll) / sum w, absolute 2^-24, extra 2 SUM_EPS + 2^-24   (numerator, denominator, store)
      ce_w / sum w   r = SUM_EPS + 2^-24;   focal_w / (N hw): one rounding, inside the 2^-22 floor
      focal      S = sum S(focal_i) / (N hw), absolute mean of the per-pixel one, extra SUM_EPS + 2^-24
      total      the weighted sum of the three (S, absolute and extra alike)
      dlogits    S = S(p_c) (G_c + sum_j G_j S(p_j)) + K (S(p_c) + h_c),  G_c = h_c |A_c| + |B_c|,
                 K = ce_w w / sum w + focal_w alpha ((1 + pt)^gamma + gamma (1 + pt)^(gamma - 1) S(pt) S(nll)) / (N hw);
                 absolute = p_c (D_c + sum_j D_j p_j) + (p_c + h_c) (r ce_w w / sum w
                            + focal_w alpha gamma (1 - pt)^(gamma - 1) pt 2^-24 / (N hw)),  D_c = h_c r_A |A_c| + r_B |B_c|
      is_prob    d = h_c A_c + B_c:  bound h_c r_A |A_c| + r_B |B_c| + 2^-24 |d| with lib = 0 (no library function),
                 returned as S = bound / SUM_EPS for assert_fp32.
    -> {'loss': (v[4], S[4]), 'loss_abs': [4], 'loss_extra': [4], 'loss_host': [4], 'dlogits': (v, S), 'dlogits_abs',
        'dlogits_host', 'A', 'B', 'ce_scale'}; images: the image indices the gradient is returned for (default all).
    defect: one of SEG_DEFECTS, the planted defects of test_cpu_ref64.py."""
    z32 = logits.detach().to(torch.float32).cpu()
    tg = target.detach().to(torch.int64).cpu()
    N, C, hw = z32.shape
    cw = None if class_weights is None else class_weights.detach().to(torch.float32).cpu()
    ce_w, dice_w, focal_w, alpha, gamma = (_f32(v) for v in (ce_w, dice_w, focal_w, alpha, gamma))
    f64, f32 = torch.float64, torch.float32
    sm = 1e-8
    I, Pp, T, Ih, Ph = (torch.zeros(N, C, dtype=f64) for _ in range(5))
    num = den = fsum = numh = fsumh = s_num = s_foc = a_num = a_foc = 0.0
    for n in range(N):
        zn, tn = z32[n], tg[n]
        if defect == "drop_block" and n == 0:            # the second 4096-pixel block (the last one if there is no other)
            keep = torch.ones(hw, dtype=torch.bool)
            b0 = min(SEG_BLOCK, max(hw - SEG_BLOCK, 0))
            keep[b0:b0 + SEG_BLOCK] = False
            zn, tn = zn[:, keep], tn[keep]
        if defect == "drop_tail" and n == 0:
            zn, tn = zn[:, :-1], tn[:-1]
        for dt_ in (f64, f32):
            q = _seg_pixels(zn, tn, C, ignore_index, cw, alpha, gamma, dt_, is_prob, defect)
            p, h = q["p"].to(f64), q["h"]
            pin = p * q["valid"] if defect == "sump_skips_ignored" else p
            if dt_ == f64:
                I[n], Pp[n], T[n] = (p * h).sum(1), pin.sum(1), h.sum(1).to(f64)
            else:
                Ih[n], Ph[n] = (p * h).sum(1), pin.sum(1)
            if is_prob:
                continue
            if dt_ == f64:
                num, den, fsum = num + float((q["w"] * q["nll"]).sum()), den + float(q["w"].sum()), fsum + float(q["foc"].sum())
                op = (1 + q["pt"]) ** gamma * q["valid"]
                s_num, a_num = s_num + float((q["w"] * q["s_nll"]).sum()), a_num + float(q["w"].sum()) * SEG_CE_ABS
                s_foc, a_foc = s_foc + float((alpha * op * q["s_nll"]).sum()), a_foc + float((alpha * op).sum()) * SEG_CE_ABS
            else:
                numh, fsumh = numh + float((q["w"].to(f64) * q["nll"].to(f64)).sum()), fsumh + float(q["foc"].to(f64).sum())
    npix = float(N) * hw
    fden = float(den) if defect == "focal_over_valid" else npix          # (unit weights: den counts the valid pixels)
    U = Pp + T + sm
    dice_nc = (2 * I + sm) / U
    lib = lambda a, b: max(4 * float(((a - b).abs() / b.clamp_min(1e-300)).max()), MEASURED_FLOOR)      # noqa: E731
    r_I, r_P = (0.0, 0.0) if is_prob else (lib(Ih, I), lib(Ph, Pp))
    r_I, r_P = r_I + SUM_EPS, r_P + SUM_EPS
    dice = 1 - dice_nc.mean()
    s_dice = 1 + (2 * I / U + dice_nc * Pp / U).mean()
    dice_h = 1 - ((2 * Ih + sm) / (Ph + T + sm)).mean()
    ce, ce_h = (num / den, numh / den) if den > 0 else (0.0, 0.0)
    s_ce, a_ce = (s_num / den, a_num / den) if den > 0 else (0.0, 0.0)
    focal, focal_h, s_focal, a_focal = fsum / fden, fsumh / fden, s_foc / fden, a_foc / fden
    wts = [w if w > 0 else 0.0 for w in (ce_w, dice_w, focal_w)]
    mix = lambda a, b, c: wts[0] * a + wts[1] * b + wts[2] * c      # noqa: E731
    e_ce, e_dice, e_focal = 2 * SUM_EPS + 2.0 ** -24, SUM_EPS + 2.0 ** -24, SUM_EPS + 2.0 ** -24
    t64 = lambda *v: torch.tensor([float(x) for x in v], dtype=f64)      # noqa: E731
    out = {"loss": (t64(mix(ce, dice, focal), ce, dice, focal), t64(mix(s_ce, s_dice, s_focal), s_ce, s_dice, s_focal)),
           "loss_abs": t64(mix(a_ce, 0.0, a_focal), a_ce, 0.0, a_focal),
           "loss_extra": t64(max(e_ce, e_dice, e_focal) + 2.0 ** -24, e_ce, e_dice, e_focal),
           "loss_host": t64(mix(ce_h, dice_h, focal_h), ce_h, dice_h, focal_h)}
    if is_prob:                                          # loss[1], loss[3] are outside the contract for a probability map
        out["loss"] = (out["loss"][0][[0, 2]], out["loss"][1][[0, 2]])
        for k in ("loss_abs", "loss_extra", "loss_host"):
            out[k] = out[k][[0, 2]]
    inv_nc = 1.0 / (N * C)
    A = -wts[1] * inv_nc * 2.0 / U
    B = wts[1] * inv_nc * (2 * I + sm) / (U * U)
    if defect == "b_sign":
        B = -B
    if defect == "a_class":
        A = A.roll(1, 1)
    r_A = r_P * Pp / U + 2.0 ** -24
    r_B = r_I * 2 * I / (2 * I + sm) + 2 * r_P * Pp / U + 2.0 ** -24
    ce_s = wts[0] / den if den > 0 else 0.0
    fo_s = wts[2] / fden
    r_den = SUM_EPS + 2.0 ** -24
    out.update(A=A, B=B, ce_scale=ce_s)
    if not grad:
        return out
    images = list(range(N)) if images is None else list(images)
    val, S, Ab, host = (torch.empty((len(images), C, hw), dtype=f64) for _ in range(4))
    for i, n in enumerate(images):
        An, Bn = A[n][:, None], B[n][:, None]
        if is_prob:
            h = _seg_pixels(z32[n], tg[n], C, ignore_index, None, alpha, gamma, f64, True)["h"].to(f64)
            val[i] = h * An + Bn
            S[i] = (h * An.abs() * r_A[n][:, None] + Bn.abs() * r_B[n][:, None] + 2.0 ** -24 * val[i].abs()) / SUM_EPS
            Ab[i], host[i] = 0.0, val[i]
            continue
        for dt_ in (f64, f32):
            q = _seg_pixels(z32[n], tg[n], C, ignore_index, cw, alpha, gamma, dt_, False, defect)
            p, h, pt, nll, om, w = q["p"], q["h"].to(dt_), q["pt"], q["nll"], q["om"], q["w"]
            a_, b_ = An.to(dt_), Bn.to(dt_)
            g = h * a_ + b_
            dterm = 0.0 if defect == "no_focal_dterm" else gamma * om ** (gamma - 1) * pt * nll
            k = torch.tensor(ce_s, dtype=dt_) * w + torch.tensor(fo_s * alpha, dtype=dt_) * (om ** gamma + dterm) * q["valid"]
            dv = p * (g - (g * p).sum(0)) + k * (p - h)
            if dt_ == f32:
                host[i] = dv.to(f64)
                continue
            val[i] = dv
            sp = p * (1 + q["d"].abs() / 4)
            G = h * An.abs() + Bn.abs()
            spt = torch.where(q["valid"], sp.gather(0, q["tc"][None])[0], torch.ones_like(pt))
            K = ce_s * w + fo_s * alpha * ((1 + pt) ** gamma + gamma * (1 + pt) ** (gamma - 1) * spt * q["s_nll"]) * q["valid"]
            S[i] = sp * (G + (G * sp).sum(0)) + K * (sp + h)
            D = h * (An.abs() * r_A[n][:, None]) + Bn.abs() * r_B[n][:, None]
            Ab[i] = p * (D + (D * p).sum(0)) + (p + h) * (r_den * ce_s * w + fo_s * alpha * gamma * om ** (gamma - 1) * pt
                                                          * SEG_CE_ABS * q["valid"])
    out.update(dlogits=(val, S), dlogits_abs=Ab, dlogits_host=host)
    return out


# ------------------------------------------------------------------ comparator
def _where(idx, shape):
    out = []
    for s in reversed(shape):
        out.append(idx % s)
        idx //= s
    return tuple(reversed(out))


def _compare(kind, out, ref, S, what, mask):
    out = out.detach().to(torch.float64).cpu().contiguous()          # (NHWC outputs: logical NCHW order)
    ref, S = ref.contiguous(), S.contiguous()
    assert out.shape == ref.shape, (what, tuple(out.shape), tuple(ref.shape))
    assert bool(torch.isfinite(out).all()), f"{what}: non-finite output"
    bound = SUM_EPS * S.to(torch.float64)
    if kind == "bf16":
        bound = bound + half_ulp_bf16(ref)
    err = (out - ref).abs()
    ratio = err / torch.where(bound > 0, bound, torch.full_like(bound, 1e-300))
    if mask is not None:
        ratio = torch.where(mask, ratio, torch.zeros_like(ratio))
    i = int(ratio.argmax())
    worst = float(ratio.view(-1)[i])
    WORST[kind] = max(WORST[kind], worst)
    if worst > 1.0:
        at = _where(i, tuple(ref.shape))
        bad = int((ratio > 1.0).sum())
        raise AssertionError(
            f"{what}: worst element {at} (n, c, y, x / co, ci, ky, kx): out {float(out.view(-1)[i]):.8e} ref "
            f"{float(ref.view(-1)[i]):.8e} err {float(err.view(-1)[i]):.3e} = {worst:.2f} x bound "
            f"{float(bound.view(-1)[i]):.3e} (S {float(S.view(-1)[i]):.3e}); {bad} of {ratio.numel()} elements over")
    return worst


def assert_bf16(out, ref_s, what, mask=None):
    """bf16-stored output (y, dx, dz): |out - ref| <= half_ulp_bf16(ref) + 2^-18 S; returns the worst err / bound"""
    ref, S = ref_s
    return _compare("bf16", out, ref, S, what, mask)


def assert_fp32(out, ref_s, what, mask=None):
    """fp32-stored output (dw, db, statistics sums): |out - ref| <= 2^-18 S; returns the worst err / bound"""
    ref, S = ref_s
    return _compare("fp32", out, ref, S, what, mask)


MEASURED = {}                 # what -> (host err / S, kernel err / S, allowed / S) of assert_measured, for the results file
MEASURED_FLOOR = 2.0 ** -22   # never ask for less than 4 fp32 roundings of S


def assert_measured(out, ref_s, host, what, extra=0.0, mask=None, absolute=0.0):
    """fp32 output of a kernel whose error is a library function's (sqrt, log, pow, a division), not a summation's: the
    oracle's fp32 CPU evaluation `host` of the same formula on the same inputs is measured against the float64 value,
    worst |err| / S, and the kernel gets 4 x that, never less than 2^-22 S (device functions are specified to 1-2 ulp
    where the host libm is within 1; fma contraction).  extra: added to the allowed ratio (SUM_EPS for reduced scalars).
    Results in fp32's denormal range are held to 2^-148 absolutely and left out of the measured ratio (a store there is
    not a relative error).  absolute: a DERIVED absolute allowance per element (seg_loss), added to the bound and taken
    off the host's error before it is measured.  Returns the worst err / bound."""
    ref, S = ref_s
    S = S.to(torch.float64)
    tiny = 2.0 ** -148                 # two stores in fp32's denormal range (half of 2^-149 each, the first carried along)
    normal = ref.abs() >= 2.0 ** -126                   # denormal results are held absolutely, and kept out of the ratio
    if mask is not None:
        normal = normal & mask
    den = torch.where(S > 0, S, torch.full_like(S, 1e-300))
    hr = torch.where(normal, ((host.detach().to(torch.float64).cpu() - ref).abs() - absolute).clamp_min(0) / den, torch.zeros_like(den))
    host_ratio = float(hr.max())
    allow = max(4 * host_ratio, MEASURED_FLOOR) + extra
    kr = torch.where(normal, (out.detach().to(torch.float64).cpu() - ref).abs() / den, torch.zeros_like(den))
    MEASURED[what] = (host_ratio, float(kr.max()), allow)
    return _compare("fp32", out, ref, (S * allow + tiny + absolute) / SUM_EPS, what, mask)


SEG_OUTPUTS = ("total", "ce", "dice", "focal")


def assert_seg(loss, dlogits, ref, what):
    """unet_seg_loss outputs against seg_loss(): the loss values one by one (each has its own S, absolute and extra) and
    every gradient element.  dlogits None: values only.  -> {output name: worst err / bound}"""
    names = SEG_OUTPUTS if ref["loss"][0].numel() == 4 else ("total", "dice")
    loss = loss.detach().to(torch.float64).cpu().reshape(-1)
    if len(names) == 2:
        loss = loss[[0, 2]]
    worst = {}
    for i, k in enumerate(names):
        worst[k] = assert_measured(loss[i:i + 1], (ref["loss"][0][i:i + 1], ref["loss"][1][i:i + 1]), ref["loss_host"][i:i + 1],
                                   f"{what}: {k} loss", extra=float(ref["loss_extra"][i]), absolute=ref["loss_abs"][i:i + 1])
    if dlogits is not None:
        d = dlogits.detach().to(torch.float64).cpu().reshape(ref["dlogits"][0].shape)
        if len(names) == 2:
            worst["dlogits"] = assert_fp32(d, ref["dlogits"], f"{what}: d dice / d map")
        else:
            worst["dlogits"] = assert_measured(d, ref["dlogits"], ref["dlogits_host"], f"{what}: dlogits",
                                               absolute=ref["dlogits_abs"])
    return worst
