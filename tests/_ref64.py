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
"""
import torch
import torch.nn.functional as F

SUM_EPS = 2.0 ** -18          # fp32 summation allowance, relative to S (64 x the 2^-24 of one fp32 rounding)
BF16_MANT = 8                 # bf16 significand bits (7 stored + the implicit one)

# the largest weight-gradient reduction length (N * H * W pixels) any bf16 test in the suite compares with the fp32
# bound: BIG_CONV_CASES (8, 128, 128, 128, 128) of test_gpu_kernels.py.  test_cpu_ref64.py plants a missing 32-pixel
# block at this K; the GPU tests assert they stay at or below it.
MAX_WGRAD_K = 8 * 128 * 128

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
def conv3x3(x, w):
    """y = conv2d(x, w, padding=1)"""
    x, w = q64(x), q64(w)
    return F.conv2d(x, w, padding=1), F.conv2d(x.abs(), w.abs(), padding=1)


def conv3x3_dgrad(dy, w):
    """dx of y = conv2d(x, w, padding=1)"""
    dy, w = q64(dy), q64(w)
    return F.conv_transpose2d(dy, w, padding=1), F.conv_transpose2d(dy.abs(), w.abs(), padding=1)


def conv3x3_wgrad(x, dy):
    """dw of y = conv2d(x, w, padding=1), dw[co, ci, ky, kx]"""
    x, dy = q64(x), q64(dy)
    shape = (dy.shape[1], x.shape[1], 3, 3)
    g = torch.nn.grad.conv2d_weight
    return g(x, shape, dy, padding=1), g(x.abs(), shape, dy.abs(), padding=1)


def convt2x2(x, w, b):
    """y = conv_transpose2d(x, w, b, stride=2); w[ci, co, 2, 2] bf16-quantised, the bias stays fp32"""
    x, w, b = q64(x), q64(w), b.detach().to(torch.float64).cpu()
    return F.conv_transpose2d(x, w, b, stride=2), F.conv_transpose2d(x.abs(), w.abs(), b.abs(), stride=2)


def convt2x2_dgrad(dy, w):
    """dx of y = conv_transpose2d(x, w, stride=2)"""
    dy, w = q64(dy), q64(w)
    return F.conv2d(dy, w, stride=2), F.conv2d(dy.abs(), w.abs(), stride=2)


def convt2x2_wgrad(x, dy):
    """(dw[ci, co, 2, 2], db[co]) of y = conv_transpose2d(x, w, b, stride=2)"""
    x, dy = q64(x), q64(dy)
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
